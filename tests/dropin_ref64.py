"""Test infrastructure: a plain float64 torch (CPU) restatement of the reference model (src/model_def.py:5-46)
as autograd modules, for the drop-in usage tests (tests/test_dropin_autograd_gpu.py). Everything is torch's
own autograd over F.conv2d / relu / F.linear / F.cross_entropy; the one difference from the reference is the
max-pool, replaced by a differentiable gather at a GIVEN routing code (pool_by_code), so that the reference
takes the same pool route as the f32 kernel it is compared with: a float64 argmax disagrees with an f32
kernel on the few windows whose top two values are a numerical tie (ref64.assert_routing_ties bounds those).
With float64's own code (ref64.routing64) the helper IS F.max_pool2d, gradients included
(tests/test_dropin_ref64_cpu.py).

The modules take the routing code as a second forward argument; otherwise they are used exactly like
splitcnn.model_def's: parameters(), .grad, requires_grad_(), zero_grad().
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

F64 = torch.float64


def pool_by_code(r, code):
    """r [B,64,24,24] float64 relu'd; code [B,64,12,12], 0-3 = window position (dy * 2 + dx), 4 = blocked."""
    B = r.shape[0]
    win = r.reshape(B, 64, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, 64, 12, 12, 4)
    g = win.gather(-1, code.clamp(max=3).long()[..., None])[..., 0]
    return torch.where(code < 4, g, torch.zeros_like(g))


def conv2_relu(x, conv2):
    return F.relu(F.conv2d(x, conv2.weight, conv2.bias))


class RefPartA(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 32, 3, 1).to(F64)

    def forward(self, x):
        return F.relu(F.conv2d(x, self.conv1.weight, self.conv1.bias))


class RefPartB(nn.Module):
    """forward(x, code): code = the routing code of this input's pool; None = float64's own max-pool."""

    def __init__(self):
        super().__init__()
        self.conv2 = nn.Conv2d(32, 64, 3, 1).to(F64)
        self.fc1 = nn.Linear(9216, 10).to(F64)

    def forward(self, x, code=None):
        r = conv2_relu(x, self.conv2)
        pooled = F.max_pool2d(r, 2) if code is None else pool_by_code(r, code)
        return F.linear(pooled.reshape(pooled.shape[0], 9216), self.fc1.weight, self.fc1.bias)


class RefFull(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 32, 3, 1).to(F64)
        self.conv2 = nn.Conv2d(32, 64, 3, 1).to(F64)
        self.fc1 = nn.Linear(9216, 10).to(F64)

    def forward(self, x, code=None):
        r = conv2_relu(F.relu(F.conv2d(x, self.conv1.weight, self.conv1.bias)), self.conv2)
        pooled = F.max_pool2d(r, 2) if code is None else pool_by_code(r, code)
        return F.linear(pooled.reshape(pooled.shape[0], 9216), self.fc1.weight, self.fc1.bias)


def cross_entropy(logits, labels):
    """nn.CrossEntropyLoss() as the reference uses it (mean, integer labels)."""
    return F.cross_entropy(logits, labels.long())


def load64(ref, *modules):
    """Copy the (f32) parameters of splitcnn modules, or of dicts name -> array, into the float64 module `ref`."""
    sd = {}
    for m in modules:
        for k, v in (m.state_dict() if isinstance(m, nn.Module) else m).items():
            sd[k] = torch.as_tensor(v).detach().to("cpu", F64)
    ref.load_state_dict(sd)
    return ref
