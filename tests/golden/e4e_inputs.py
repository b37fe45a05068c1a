"""Inputs of the e4e fixture (tests/golden/e4e.npz), shared by make_golden_e4e.py and the tests: drawn by a seeded
torch.Generator, so they are regenerated and never stored."""
import torch

SEED = 5                                  # synthetic.e4e_state_dict(net, seed=SEED)
CASES = {"64": (2, 64), "256": (1, 256)}   # fixture key -> (n, size)
ENCODERS = ("Encoder4Editing", "GradualStyleEncoder")


def e4e_input(n, size):
    g = torch.Generator().manual_seed(1000 + size)
    return torch.randn(n, 3, size, size, generator=g).clamp_(-1, 1)
