"""Reference and fixtures for the direct tests of the NHWC BatchNorm backward kernels
(tests/test_bn_kernels_cpu.py, tests/test_gpu_bn_kernels.py).

Written from the contract in include/gsync.h; nothing here calls the library.

* ``bn_bwd_ref``: the backward in fp64 (torch, on whatever device its inputs live on).
* bf16 bit helpers: ``bf16_bits``, ``trunc_bf16``, ``ulp_bf16``.
* ``exact_inputs``: inputs on a grid of small dyadic values.  With them every sum the
  kernels form is exact in fp32 in any order (and, for R a power of two, every step of the
  dx chain), so the kernels' results must equal the fp64 reference bit for bit
  (test_bn_kernels_cpu.py asserts the condition for every shape in the lists below).
* ``guarded`` / ``guards_intact``: a tensor inside a larger buffer whose margins hold a
  NaN pattern no kernel produces, to see a store outside the buffer.
"""
import math

import torch

# ---- the shapes of the exact grid (R rows, C channels) -------------------------------------
# dx is compared bitwise where R is a power of two (sum / R is then exact)
BITWISE_DX_SHAPES = [
    (1, 8),        # one row
    (2, 8),        # two rows
    (64, 8),       # tx = 1, ty = 256
    (256, 64),     # tx = 8
    (1024, 16),    # tx = 2
    (1024, 72),    # two tiles, the second has one live vector
    (4096, 40),    # three dead vectors, P = 45
    (512, 520),    # nine tiles with a ragged last one
    (1024, 2048),  # 32 tiles, the ctiles * P > 256 adjustment
]
# the sums are compared bitwise, dx by the derived bound
SUM_SHAPES = [
    (255, 8),       # P = 1
    (257, 8),       # P = 2, uneven last block
    (1027, 8),
    (20000, 8),     # P = 79 > G4 = 64: the fold's strided loop wraps
    (777, 24),      # tx = 4 with a dead vector
    (8191, 64),
    (20000, 256),   # P adjusted to 64, rpb = 313: two unrolled iterations plus a ragged tail
    (400, 2048),
    (196, 2048),
    (3000, 1032),
    (600000, 8),    # tx = 1 through the unrolled loop
]
EXACT_SHAPES = BITWISE_DX_SHAPES + SUM_SHAPES
VARIANTS = ["plain", "relu", "add_relu"]

WEIGHT_CYCLE = (-0.75, 0.0, 0.5, 1.0, 1.5, 2.0, -1.25)
U32 = 2.0 ** -24  # unit roundoff of fp32


def exact_seed(R, C):
    return 7919 + (R % 100003) * 31 + C


def shape_id(s):
    return f"{s[0]}x{s[1]}"


# ---- the reference ---------------------------------------------------------------------------
def bn_bwd_ref(x, dy, y, mean, invstd, weight):
    """fp64 BatchNorm backward over a row-major [R, C] activation.

    g = where(y <= 0, 0, dy) (a NaN y passes dy; y None: g = dy)
    sum_g = sum g, sum_gx = sum g * (x - mean) (what the workspace holds, before invstd)
    gw = invstd * sum_gx, gb = sum_g
    dx = w * invstd * (g - sum_g / R - (x - mean) * invstd^2 * sum_gx / R)
    Returns g, sum_g, sum_gx, gw, gb, dx, all fp64."""
    xd, g = x.double(), dy.double()
    R = xd.shape[0]
    if y is not None:
        g = torch.where(y.double() <= 0, torch.zeros_like(g), g)
    m, s, w = mean.double(), invstd.double(), weight.double()
    xc = xd - m
    sum_g = g.sum(0)
    sum_gx = (g * xc).sum(0)
    m1 = sum_g / R
    k2 = s * s * sum_gx / R
    dx = w * s * (g - m1 - xc * k2)
    return g, sum_g, sum_gx, s * sum_gx, sum_g, dx


# ---- bf16 bits ---------------------------------------------------------------------------------
def bf16_bits(t):
    """the bf16 patterns of t as int16 (a tensor of another dtype is converted to bf16 first)"""
    if t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    return t.contiguous().view(torch.int16)


def from_bits(bits, device="cpu"):
    """bf16 tensor from a list of 16-bit patterns"""
    b = torch.tensor([v - 65536 if v >= 32768 else v for v in bits], dtype=torch.int16, device=device)
    return b.view(torch.bfloat16)


def trunc_bf16(v):
    """fp64 -> fp32 (round to nearest) -> bf16 toward zero: the low 16 bits of the fp32 pattern masked"""
    i = v.to(torch.float32).contiguous().view(torch.int32) & -65536
    return i.view(torch.float32).to(torch.bfloat16)  # exact: the low mantissa bits are zero


def ulp_bf16(v):
    """the spacing of bf16 at |v| (fp64 tensor): 2^(floor(log2 |v|) - 7), the subnormal spacing below 2^-126"""
    a = v.double().abs()
    _, e = torch.frexp(a)  # |v| = m * 2^e, m in [0.5, 1); frexp(0) = (0, 0)
    e = torch.where(a == 0, torch.full_like(e, -126), torch.clamp(e - 1, min=-126)) - 7
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e)


def is_f32(v):
    """elementwise: the fp64 value is representable in fp32"""
    return v.to(torch.float32).double() == v


# ---- inputs on the exact grid --------------------------------------------------------------------
def exact_inputs(R, C, seed=None):
    """CPU tensors x, dy, y (bf16 [R, C]) and mean, invstd, weight (fp32 [C]).

    mean_c = ((5c mod 17) - 8) / 2, invstd_c = 2^((c mod 3) - 1), weight_c = WEIGHT_CYCLE[c mod 7]:
    cycle lengths coprime with 8 and with 64, so channels swapped inside a vector or a tile show.
    x = mean + e, e uniform on {-2, -1.5, ..., 2}; dy uniform on the multiples of 0.25 in [-2, 2];
    y uniform on {-1, 0, 1}.  Every value is a bf16."""
    gen = torch.Generator().manual_seed(exact_seed(R, C) if seed is None else seed)
    c = torch.arange(C)
    mean = (((5 * c) % 17) - 8).to(torch.float32) * 0.5
    invstd = torch.ldexp(torch.ones(C), (c % 3) - 1).to(torch.float32)
    weight = torch.tensor(WEIGHT_CYCLE, dtype=torch.float32)[c % 7]
    e = (torch.randint(0, 9, (R, C), generator=gen) - 4).to(torch.float32) * 0.5
    x = (mean + e).to(torch.bfloat16)
    dy = ((torch.randint(0, 17, (R, C), generator=gen) - 8).to(torch.float32) * 0.25).to(torch.bfloat16)
    y = (torch.randint(0, 3, (R, C), generator=gen) - 1).to(torch.bfloat16)
    return dict(x=x, dy=dy, y=y, mean=mean, invstd=invstd, weight=weight)


def random_inputs(R, C, seed):
    """Tier B: x = bf16(randn * sc_c + mu_c), mu_c over [-8, 8], sc_c over [0.25, 4]; mean / invstd the
    fp64 batch statistics of that bf16 x (eps 1e-5) rounded to fp32; weights with a negative and a zero;
    dy = bf16(randn); y bf16, about half positive, about 6 % exact zeros."""
    gen = torch.Generator().manual_seed(seed)
    mu = torch.linspace(-8.0, 8.0, C)
    sc = torch.logspace(math.log10(0.25), math.log10(4.0), C).flip(0)
    x = (torch.randn(R, C, generator=gen) * sc + mu).to(torch.bfloat16)
    xd = x.double()
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    w = torch.empty(C).uniform_(0.5, 1.5, generator=gen)
    w[0], w[1] = -0.75, 0.0
    dy = torch.randn(R, C, generator=gen).to(torch.bfloat16)
    y = torch.randn(R, C, generator=gen).to(torch.bfloat16)
    y[torch.rand(R, C, generator=gen) < 0.06] = 0.0
    return dict(x=x, dy=dy, y=y, mean=mean.to(torch.float32), invstd=invstd.to(torch.float32), weight=w)


# ---- guarded buffers -------------------------------------------------------------------------------
GUARD_BYTES = 4096
LINE_BYTES = 128
_PATTERN = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float32: (torch.int32, 0x7FC00001)}


def guarded(n, dtype, device, offset_elems=0):
    """A view of n elements inside a larger buffer: at least 4 KiB of guard on each side, the whole
    buffer (view included) filled with the bit pattern 0x7FC1 (bf16) / 0x7FC00001 (fp32), the view
    starting offset_elems past a 128-byte line (so offset_elems * itemsize must be a multiple of 16
    for a 16-byte aligned view).  guards_intact(view) tells whether the margins are untouched."""
    itype, pat = _PATTERN[dtype]
    size = torch.empty(0, dtype=dtype).element_size()
    g = GUARD_BYTES // size
    total = g + LINE_BYTES // size + offset_elems + n + g
    raw = torch.empty(total, dtype=itype, device=device)
    raw.fill_(pat)
    assert raw.data_ptr() % size == 0
    start = g
    while (raw.data_ptr() + start * size) % LINE_BYTES:
        start += 1
    start += offset_elems
    view = raw.view(dtype)[start:start + n]
    assert view.data_ptr() == raw.data_ptr() + start * size and view.data_ptr() % LINE_BYTES == (
        offset_elems * size) % LINE_BYTES
    view._bn_guard = (raw, start, n, pat)
    return view


def guards_intact(view):
    raw, start, n, pat = view._bn_guard
    return bool((raw[:start] == pat).all()) and bool((raw[start + n:] == pat).all())


def bits(t):
    """the tensor's bit patterns as integers (for bitwise comparisons that treat NaNs and zeros as data)"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
