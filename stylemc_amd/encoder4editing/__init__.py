"""e4e real-image inversion (image -> W+), laid out as the reference's ``encoder4editing/`` package: ``infer`` is the CLI,
``models.encoders`` the torch restatement of the encoders; the GPU executor is ``stylemc_amd.e4e_hip``."""
