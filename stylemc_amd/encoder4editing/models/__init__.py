"""``encoder4editing/models`` of the reference: the encoders (the rosinality decoder is not needed to write W)."""
