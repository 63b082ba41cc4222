"""fp64 restatement of torch.optim.Muon's formulae (T:optim/_muon.py) and the shape list
the Muon tests share.  A parameter is taken as the row-major [shape[0], numel/shape[0]]
matrix in memory order, as FusedMuon takes it."""
import math

import torch
from torch.optim._muon import _zeropower_via_newtonschulz

COEF = (3.4445, -4.7750, 2.0315)
# an exact tile, odd n, transposed tensors, m one past a tile, three tiles with a remainder
# of one, a channels_last and a contiguous filter; one list, so the grouped launches see
# mixed shapes at once
SHAPES = [(32, 32), (64, 147), (96, 40), (33, 65), (200, 72), (130, 300), (257, 260), "cl:48,16,3,3", (16, 8, 3, 3)]
CPU_SHAPES = [(96, 40), (33, 65), "cl:48,16,3,3"]


def make(shape, device, gen, dtype=torch.float32):
    """A random normal tensor of an entry of SHAPES on ``device`` (generated on the CPU)."""
    cl = isinstance(shape, str)
    dims = tuple(int(v) for v in shape[3:].split(",")) if cl else shape
    t = torch.randn(dims, generator=gen).to(dtype)
    return (t.contiguous(memory_format=torch.channels_last) if cl else t).to(device)


def matrix(t):
    """The [A, B] matrix FusedMuon sees: the tensor's memory order, fp64, on the CPU."""
    t = t.detach()
    if t.ndim == 4 and not t.is_contiguous():
        t = t.permute(0, 2, 3, 1)
    return t.reshape(t.shape[0], -1).double().cpu()


def newton_schulz(u, steps, eps, coef=COEF):
    a, b, c = coef
    x = u.T if u.shape[0] > u.shape[1] else u
    x = x / x.norm().clamp(min=eps)
    for _ in range(steps):
        g = x @ x.T
        x = a * x + (b * g + c * (g @ g)) @ x
    return x.T if u.shape[0] > u.shape[1] else x


def direction(g, buf, momentum, nesterov):
    """(new buffer, update direction u) from the grad and the old buffer."""
    buf = buf + (1 - momentum) * (g - buf)
    return buf, (g + momentum * (buf - g) if nesterov else buf)


def adjusted_lr(lr, fn, A, B):
    return lr * (0.2 * math.sqrt(max(A, B)) if fn == "match_rms_adamw" else math.sqrt(max(1, A / B)))


def rel_err(x, ref):
    return float((x.double().cpu() - ref).norm() / ref.norm())


def torch_ns_err(u, steps, eps, device):
    """torch's own bf16 Newton-Schulz on the same u on ``device``, against fp64."""
    o = _zeropower_via_newtonschulz(u.float().to(device), COEF, steps, eps)
    return rel_err(o, newton_schulz(u, steps, eps))


def fused_x(plan, ws, t, xsel, A, B):
    """Tensor t's X buffer ``xsel`` of the workspace in the parameter's orientation, fp64."""
    lay = plan._muon["tensors"][t]
    off = lay["x1" if xsel else "x0"]
    x = ws[off:off + lay["lda"] * lay["ldx"]].view(lay["lda"], lay["ldx"])[:lay["m"], :lay["n"]].double().cpu()
    return x.T if A > B else x
