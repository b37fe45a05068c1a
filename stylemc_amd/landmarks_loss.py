"""The two landmark distances of the reference's landmarks_loss.py, on [batch, 68, 2] point sets.  Both drop the 17
jaw-line points (indices 0..16) and compare the remaining 51."""
import math

import torch
import torch.nn.functional as F
from torch import nn

JAW_POINTS = 17


class LandmarksLoss(nn.Module):
    """Mean squared coordinate difference (landmarks_loss.py:34-46); the term find_direction prints."""

    def forward(self, landmarks1, landmarks2):
        return F.mse_loss(landmarks1[:, JAW_POINTS:].reshape(-1, 2), landmarks2[:, JAW_POINTS:].reshape(-1, 2))


class WingLoss(nn.Module):
    """Wing loss (landmarks_loss.py:10-31): omega * log(1 + d / epsilon) for coordinate differences d below omega, d - C
    above, with C = omega - omega * log(1 + omega / epsilon) joining the two pieces; the mean over all coordinates."""

    def __init__(self, omega=10, epsilon=2):
        super().__init__()
        self.omega = omega
        self.epsilon = epsilon

    def forward(self, landmarks1, landmarks2):
        d = (landmarks1[:, JAW_POINTS:].reshape(-1, 2) - landmarks2[:, JAW_POINTS:].reshape(-1, 2)).abs()
        small, large = d[d < self.omega], d[d >= self.omega]
        c = self.omega - self.omega * math.log(1 + self.omega / self.epsilon)
        total = (self.omega * torch.log(1 + small / self.epsilon)).sum() + (large - c).sum()
        return total / (small.numel() + large.numel())
