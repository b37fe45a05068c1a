"""``encoder4editing/models/encoders`` of the reference."""
