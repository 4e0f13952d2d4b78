"""Stand-ins for the networks of the synchronisation layer (the WAM embedder / extractor and the SyncSeal TorchScript are not part of
this repository): just enough to drive WamSync / SyncSeal / the harness end to end with known answers."""
import torch

from tests import sync_cases as SC

MEAN = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)


class ColourWam:
    """A WAM-like object that "embeds" message k as the flat colour sync_cases.COLOURS[k] and "detects" by classifying colours back:
    a pixel within 0.3 (WAM-normalised units, per channel) of a colour gets mask logit +8 and that message's bit logits +-8, any other
    pixel mask logit -8.  Pointwise and far from every decision edge, so CPU and GPU agree exactly."""

    def __init__(self, device):
        self.device = device
        self.colours = ((torch.from_numpy(SC.COLOURS).view(4, 3, 1, 1) + 1.0) / 2.0 - MEAN[0]) / STD[0]      # WAM space, [4, 3, 1, 1]
        self.colours = self.colours.to(device)
        self.msgs = torch.from_numpy(SC.MSGS).to(device)
        self.detect_calls = 0

    def embed(self, imgs, msg):
        k = (msg[:, 0] * 2 + msg[:, 16]).long()          # the four fixed messages differ in bits 0 and 16
        return {"imgs_w": self.colours[k].expand(-1, -1, imgs.shape[-2], imgs.shape[-1]).to(imgs.dtype).contiguous()}

    def detect(self, imgs):
        self.detect_calls += 1
        d = (imgs[:, None] - self.colours[None]).abs().amax(dim=2)          # [B, 4, H, W]
        near, k = d.min(dim=1)
        bits = (self.msgs[k].permute(0, 3, 1, 2).float() * 2.0 - 1.0) * 8.0   # [B, 32, H, W]
        mask = torch.where(near < 0.3, 8.0, -8.0).unsqueeze(1)
        return {"preds": torch.cat([mask, bits], dim=1).float()}


class TinySeal(torch.nn.Module):
    """The three calls SyncSeal makes on its TorchScript: embed adds a constant, detect returns corner points, unwarp undoes embed."""

    @torch.jit.export
    def embed(self, imgs):
        return {"imgs_w": imgs * 0.5 + 0.125}

    @torch.jit.export
    def detect(self, imgs):
        return {"preds_pts": torch.zeros(imgs.shape[0], 8) + imgs.mean()}

    @torch.jit.export
    def unwarp(self, imgs, pts, size: "tuple[int, int]"):
        return (imgs - 0.125) * 2.0 + pts.sum() * 0.0

    def forward(self, imgs):
        return imgs
