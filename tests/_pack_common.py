"""Shared by tests/test_pack_variants_cpu.py (host backend) and tests/test_gpu_pack_variants.py (the
HIP kernels): the four ops of the chunk engine that every DDP and ZeRO step runs — PackOp, UnpackOp
(with its fused Σg² and its fused non-finite check), SqnormOp and ClipScaleOp — against a plain
reference, bit for bit, on guarded tensors and a guarded bucket.  Every driver takes a device, so one
body serves both backends.

No tolerance appears below.  Every comparison is exact, and may be, because
  * a pack is at most one IEEE fp32 multiply or divide (the library is built with -ffp-contract=off
    and no fast-math) between round-to-nearest-even casts, which numpy and torch's CPU kernels
    compute the same way; an unpack is one such cast;
  * the Σg² inputs are integers in [-v, v] with 2 * v² * numel < 2^24: every fp32 partial sum, in any
    order and through fmaf, is an integer below 2^24 and so exact — twice over, for the accumulating
    launch.  The fused ticket, the combine launch, the raw partials and the group sums therefore all
    equal the fp64 sum;
  * the clip coefficient is restated in numpy fp32, operation for operation (sqrt, add, divide).
Where both sides hold a NaN the comparison accepts any payload (same_bits_nan), except in bf16, where a
stored NaN is exactly 0x7FC0 (oracle.f32_to_bf16); everywhere else it is bit equality.

The bucket gets the treatment tests/_update_common.py gives a tensor (GuardedFlat): the flat pointer
is a slice of a raw buffer filled with a NaN sentinel, and after every launch every element outside
the tensors' [offset, offset + numel) ranges — the guards and the plan's alignment padding — must
still hold it.  A kernel that reads the padding poisons its sum or sets its flag; one that writes it
changes the pattern."""
import contextlib
import math

import numpy as np
import torch

from oracle import oracle as O
from tests._update_common import (BF16, DT_IDS, DTYPES, F16, F32, G, LIST_A, LIST_B, ODD_BITS,  # noqa: F401
                                  OFF_SLOT_NUMELS, PATTERN, GuardedList, _scalar, _sync, _values, assert_lists, bits,
                                  run_guarded, same_bits, same_bits_nan, sentinel_list, unscale_placements)

MODES = ["none", "mul", "div"]
SCALE = {"none": 1.0, "mul": float(np.float32(1.0 / 3.0)), "div": 3.0}
PAIRS = [(a, b) for a in DTYPES for b in DTYPES]
PAIR_IDS = [f"{a}-{b}" for a in DT_IDS for b in DT_IDS]
# a full-chunk tensor, one with full chunks and a tail, and two tails, as indices into LIST_A
NULL_A = [LIST_A.index(n) for n in (1, 5, 4096, 4097)]
# more than kPackG2MaxChunks = 4096 chunks: the one-chunk fp32 pack, the group-sums form of
# gs_sqnorm_partial_out; a tail behind it and a tiny tensor
LARGE = [4096 * 1024, 1025, 7]
assert sum(-(-n // 1024) for n in LARGE) > 4096


class GuardedFlat:
    """A plan's bucket: the slice ``raw[G+off : G+off+flat_numel]`` of a raw integer buffer whose
    every other element, and every element of the slice outside the tensors' ranges (the plan's
    alignment padding), holds the dtype's sentinel.  ``off = 1`` puts the slice one element off
    16 bytes (``flat_vec`` false)."""

    def __init__(self, plan, dtype, device, off=0):
        self.dtype, self.device = dtype, device
        self.itype, self.pat = PATTERN[dtype]
        n = plan.flat_numel
        self.raw = torch.empty(G + off + n + G, dtype=self.itype, device=device)
        self.flat = self.raw.view(dtype)[G + off:G + off + n]
        assert self.raw.data_ptr() % 16 == 0 and (n == 0 or (self.flat.data_ptr() % 16 == 0) == (off == 0))
        self.ranges = [(G + off + o, G + off + o + m) for o, m in zip(plan.offsets, plan.numels)]
        assert all(G + off <= a <= b <= G + off + n for a, b in self.ranges)
        self.pad_mask = torch.ones(self.raw.numel(), dtype=torch.bool)
        for a, b in self.ranges:
            self.pad_mask[a:b] = False

    def fill(self, values=None):
        """values: one CPU tensor of the bucket's dtype per plan tensor, or None for a range that
        keeps the sentinel; None leaves the sentinel everywhere"""
        host = torch.full((self.raw.numel(),), self.pat, dtype=self.itype)
        for (a, b), x in zip(self.ranges, values or []):
            if x is not None:
                assert x.dtype == self.dtype and x.numel() == b - a
                host[a:b] = bits(x)
        self.raw.copy_(host.to(self.device))

    def read(self):
        """(the tensors' ranges on the CPU, whether every other element still holds the sentinel)"""
        host = self.raw.cpu()
        intact = bool((host[self.pad_mask] == self.pat).all())
        return [host[a:b].clone().view(self.dtype) for a, b in self.ranges], intact


@contextlib.contextmanager
def _bound(device, numels, align, lists, null=()):
    """a plan of ``numels`` whose slot s holds ``lists[s]``'s guarded tensors, NULL for the tensors
    in ``null``"""
    from distributed_training_amd.multi_tensor import TensorListPlan

    plan = TensorListPlan(numels, device, align=align)
    try:
        for s, gl in enumerate(lists):
            plan.set_ptrs(s, [None if t in null else v for t, v in enumerate(gl.views)])
        yield plan
        _sync(device)
    finally:
        plan.close()


def _read_intact(gl, what):
    values, intact = gl.read()
    assert intact, f"{what}: an element outside the tensors changed"
    return values


def _ints(numels, dt, vmax, seed):
    """integers in [-vmax, vmax], exact in every dtype here; asserts that sums of their squares stay exact"""
    assert 2 * vmax * vmax * sum(numels) < 2 ** 24, "partial sums (of two launches) must stay exact in fp32"
    gen = torch.Generator().manual_seed(seed)
    return [torch.randint(-vmax, vmax + 1, (n,), generator=gen).to(dt) for n in numels]


# Values at which a cast or a scale goes wrong first: signed zeros, fp32 denormals, values that
# overflow 16 bits, the non-finite ones, the largest fp16 and the tie above it (65520 rounds to inf),
# ties of the bf16 cast (1 + 2^-8 rounds down to even, 1 + 3 * 2^-8 up), the smallest fp16 subnormal,
# half of it (a tie that rounds to 0) and just above that (rounds up to the subnormal)
SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 3e38, -3e38, math.inf, -math.inf, math.nan, 65504.0, 65520.0, -65519.0,
            1.00390625, 1.01171875, 2.0 ** -24, 2.0 ** -25, -(2.0 ** -25) * 1.0001, 1e-30]
# the whole list at the start of a tail tensor, of tensors with full chunks and a tail, of a full-chunk
# tensor (the vector path at plan alignment 64), and once more at the end of the 4097-element one
SPECIAL_NUMELS = (len(SPECIALS) + 3, 1025, 4097, 1, 4096)


def _special_values(dt, seed):
    x = [t.clone() for t in _values(SPECIAL_NUMELS, F32, seed)]
    sp = torch.tensor(SPECIALS)
    for t in (0, 1, 2, 4):
        x[t][:len(SPECIALS)] = sp
    x[2][-len(SPECIALS):] = sp
    x[3][0] = math.nan
    return [t.to(dt) for t in x]


# -------------------------------------------------------------------- pack
def _from_f32(a, fd):
    """The round-to-nearest-even cast of an fp32 numpy array: torch's.  For bf16 the oracle's, which
    pins a NaN to 0x7FC0 (torch's CPU cast gives 0x7FC0 or 0xFFFF, by the code path it takes); torch's
    must agree with it everywhere else."""
    out = torch.from_numpy(a).to(fd)
    if fd == BF16:
        pinned = torch.from_numpy(O.f32_to_bf16(np.ascontiguousarray(a)).view(np.int16).copy()).view(BF16)
        assert same_bits_nan(out, pinned)
        return pinned
    return out


def pack_ref(x, fd, mode):
    """NONE: the cast; MUL: one fp32 multiply, the cast; DIV: the cast, one fp32 divide, the cast
    (torch's bf16_compress_hook order)"""
    a = x.float().numpy()
    s = np.float32(SCALE[mode])
    assert float(s) == SCALE[mode] and s > 0, "the scale must be an fp32 value: the C ABI takes a float"
    if mode == "mul":
        a = a * s
    elif mode == "div":
        a = _from_f32(a, fd).float().numpy() / s
    return _from_f32(a, fd)


def run_pack(device, numels, sd, fd, mode, align=0, src_off=0, flat_off=0, null=(), seed=61):
    """gs_pack of guarded ``sd`` tensors into a guarded ``fd`` bucket pre-filled with the sentinel:
    every tensor's range holds :func:`pack_ref` bit for bit (that of zeros for a NULL source), every
    other element of the bucket still holds the sentinel, and the sources are unchanged.
    ``numels`` = SPECIAL_NUMELS: the sources hold SPECIALS; a NaN packed into a bf16 bucket is
    exactly 0x7FC0, into another dtype any NaN."""
    from distributed_training_amd import _lib as L

    numels = tuple(numels)
    x = _special_values(sd, seed) if numels == SPECIAL_NUMELS else _values(numels, sd, seed)
    want = [pack_ref(torch.zeros_like(t) if k in null else t, fd, mode) for k, t in enumerate(x)]
    for k in null:  # +0, 0 * s, 0 / s with s > 0: all +0
        assert not bits(want[k]).any()
    src = GuardedList(numels, sd, device, src_off)
    src.fill(x)
    with _bound(device, numels, align, [src], null) as plan:
        flat = GuardedFlat(plan, fd, device, flat_off)
        flat.fill(None)
        plan.pack(0, sd, flat.flat, SCALE[mode], getattr(L, "GS_SCALE_" + mode.upper()))
    assert_lists(_read_intact(flat, "bucket"), want, f"pack {mode}", nan_ok=fd != BF16)
    assert_lists(_read_intact(src, "sources"), x, "sources (read-only)", nan_ok=False)


# ------------------------------------------------------------------ unpack
def _check_unpacked(dst, flat, vals, dd, null):
    """the destinations are the cast of their bucket ranges (a NULL one untouched), the bucket is unchanged"""
    want = [_from_f32(v.float().numpy(), dd) for v in vals]
    for k, s in enumerate(sentinel_list(dst.numels, dd)):
        if k in null:
            want[k] = s
    got = _read_intact(dst, "destinations")
    for k, (a, w) in enumerate(zip(got, want)):
        exact = k in null or dd == BF16 or not torch.isnan(w.float()).any()  # a bf16 NaN is 0x7FC0
        assert (same_bits if exact else same_bits_nan)(a, w), f"unpack: tensor {k} ({a.numel()} elements) differs"
    kept = [None if k in null else v for k, v in enumerate(vals)]
    now = _read_intact(flat, "bucket")
    for k, (a, v) in enumerate(zip(now, kept)):
        assert same_bits(a, sentinel_list([a.numel()], flat.dtype)[0] if v is None else v), f"bucket range {k} changed"
    return kept


def run_unpack(device, numels, fd, dd, align=0, dst_off=0, flat_off=0, sqnorm=False, null=(), vmax=8, seed=71):
    """gs_unpack of a guarded ``fd`` bucket into guarded ``dd`` tensors.  Without ``sqnorm``: random
    values (SPECIALS with ``numels`` = SPECIAL_NUMELS; a NaN unpacked into bf16 is exactly 0x7FC0).
    With it: integers, Σ round_to<dd>(v)² onto a preset junk value — exactly the fp64 sum S — and once
    more with ``accumulate`` — exactly 2 S.  The bucket's padding, and the range of a NULL
    destination, hold NaN: neither may reach the sum."""
    numels = tuple(numels)
    if sqnorm:
        vals = _ints(numels, fd, vmax, seed)
    else:
        vals = _special_values(fd, seed) if numels == SPECIAL_NUMELS else _values(numels, fd, seed)
    fill = [None if k in null else v for k, v in enumerate(vals)]
    want_sq = float(sum((v.float().to(dd).double() ** 2).sum() for v in fill if v is not None))
    dst = GuardedList(numels, dd, device, dst_off)
    out = GuardedList([1], F32, device)
    out.fill([torch.tensor([12345.0])])
    with _bound(device, numels, align, [dst], null) as plan:
        flat = GuardedFlat(plan, fd, device, flat_off)
        flat.fill(fill)
        for acc in ([False, True] if sqnorm else [False]):
            dst.fill(None)
            plan.unpack(flat.flat, 0, dd, sqnorm=out.views[0] if sqnorm else None, accumulate=acc)
            _sync(device)
            _check_unpacked(dst, flat, vals, dd, null)
            (sq,) = _read_intact(out, "the sum's output")
            want = 12345.0 if not sqnorm else (2 * want_sq if acc else want_sq)
            assert float(sq[0]) == want, (float(sq[0]), want, acc)


def run_unpack_check(device, numels, fd, dd, align=0, nonfinite=False, null=(), seed=72):
    """gs_unpack_check.  Clean data: a flag preset to 0 stays 0 and one preset to 1 stays 1 — with
    NaN sentinels in the bucket's padding, its guards and the range of a NULL destination.  Else one
    non-finite bucket value per launch at each of :func:`unscale_placements`: the flag is exactly 1
    and every destination element is still the cast of its bucket element."""
    numels = tuple(numels)
    vals = _values(numels, fd, seed)
    dst = GuardedList(numels, dd, device)
    with _bound(device, numels, align, [dst], null) as plan:
        flat = GuardedFlat(plan, fd, device)

        def once(v, preset):
            dst.fill(None)
            flat.fill([None if k in null else a for k, a in enumerate(v)])
            flag = GuardedList([1], F32, device)
            flag.fill([torch.tensor([preset])])
            plan.unpack_check(flat.flat, 0, dd, flag.views[0])
            _sync(device)
            _check_unpacked(dst, flat, v, dd, null)
            return float(_read_intact(flag, "the flag")[0][0])

        if not nonfinite:
            for preset in (0.0, 1.0):
                assert once(vals, preset) == preset
            return
        for t, i, val in unscale_placements(numels):
            bad = [a.clone() if k == t else a for k, a in enumerate(vals)]
            bad[t][i] = val
            assert once(bad, 0.0) == 1.0, (t, i, val)


def run_unpack_check_f16_overflow(device, fd):
    """A finite bucket value that overflows an fp16 destination sets the flag: the kernel tests the
    value it stores, round_to<F16>(v).  This is the opposite of
    tests/_update_common.py::run_unscale_f16_overflow, where gs_unscale_check tests the grad it read
    (as torch's kernel does) and an overflowing product leaves the flag at 0.  60000 stays finite in
    fp16 and leaves the flag alone; 60000 * 2 does not."""
    numels = (5, 1025, 4097, 1)
    vals = [t.clone().clamp_(-100, 100) for t in _values(numels, fd, 73)]
    dst = GuardedList(numels, F16, device)
    with _bound(device, numels, 0, [dst]) as plan:
        flat = GuardedFlat(plan, fd, device)
        for big, want_flag in ((60000.0, 0.0), (120000.0, 1.0), (-120000.0, 1.0)):
            for t, i in ((2, 4096), (0, 0)):
                v = [a.clone() for a in vals]
                v[t][i] = big
                assert math.isfinite(float(v[t][i])) and abs(float(v[t][i])) >= 59000.0
                dst.fill(None)
                flat.fill(v)
                flag = _scalar(device, 0.0)
                plan.unpack_check(flat.flat, 0, F16, flag)
                _sync(device)
                _check_unpacked(dst, flat, v, F16, ())
                assert math.isinf(float(dst.read()[0][t][i])) == (want_flag == 1.0)
                assert float(flag.cpu()[0]) == want_flag, (big, t, i)


# ------------------------------------------------------------------ sqnorm
def run_sqnorm_exact(device, numels, dt, off, vmax=8, seed=81):
    """gs_sqnorm of bounded integers: exactly the fp64 sum S onto a preset junk value, exactly 2 S
    with ``accumulate``.  gs_sqnorm_partial_out on the same tensors: n in [1, GS_RED_PARTIALS], the
    fp64 sum of groups[:n] is S, groups[n:] is all +0 after a pre-fill with junk; n == 1 on the host."""
    from distributed_training_amd import _lib as L

    numels = tuple(numels)
    x = _ints(numels, dt, vmax, seed)
    want = float(sum((t.double() ** 2).sum() for t in x))
    out = GuardedList([1], F32, device)
    out.fill([torch.tensor([12345.0])])
    groups = GuardedList([L.GS_RED_PARTIALS], F32, device)
    groups.fill([torch.full((L.GS_RED_PARTIALS,), 7.0)])
    seen = []

    def launch(plan):
        for acc in (False, True):
            plan.sqnorm(0, dt, out.views[0], accumulate=acc)
            _sync(device)
            seen.append(float(_read_intact(out, "the sum's output")[0][0]))
        seen.append(plan.sqnorm_partial_out(0, dt, groups.views[0]))

    (got,) = run_guarded(device, numels, [(dt, x, off)], launch)
    assert_lists(got, x, "sqnorm input (read-only)", nan_ok=False)
    assert seen[:2] == [want, 2 * want], (seen, want)
    n = seen[2]
    (part,) = _read_intact(groups, "the partial sums")
    assert 1 <= n <= L.GS_RED_PARTIALS and (n == 1 or torch.device(device).type == "cuda"), n
    assert float(part[:n].double().sum()) == want, (n, float(part[:n].double().sum()), want)
    assert not bits(part[n:]).any(), "partial sums past n must be +0"
    return n


def run_sqnorm_empty(device, numels):
    """a plan without elements writes 0 without ``accumulate`` and leaves the output alone with it"""
    out = GuardedList([1], F32, device)
    out.fill([torch.tensor([12345.0])])

    def launch(plan):
        plan.sqnorm(0, F32, out.views[0], accumulate=True)
        _sync(device)
        assert same_bits(out.read()[0][0], torch.tensor([12345.0]))
        plan.sqnorm(0, F32, out.views[0])

    run_guarded(device, tuple(numels), [(F32, [torch.zeros(0)] * len(numels), 0)], launch)
    (val,) = _read_intact(out, "the sum's output")
    assert same_bits(val, torch.tensor([0.0]))


# -------------------------------------------------------------- clip-scale
CLIP = dict(max_norm=1.0, eps=1e-6)
SQ_CLIPS, SQ_COEF_ONE = 123.456, 0.01


def run_clip_scale(device, numels, dt, off, sq, seed=91):
    """gs_clip_scale from a supplied Σg².  Restated in numpy fp32: norm = sqrt(f32(sq)),
    c = f32(max) / (norm + f32(eps)), the coefficient 1 if c >= 1 else c; the grads are
    (x * coef) cast back, ``out`` is [sq, coef, norm], all bit for bit.  With a coefficient of 1
    nothing is written: planted NaN payloads survive."""
    numels = tuple(numels)
    x = [t.clone() for t in _values(numels, dt, seed)]
    sq32 = np.float32(sq)
    norm = np.sqrt(sq32)
    c = np.float32(CLIP["max_norm"]) / (norm + np.float32(CLIP["eps"]))
    coef = np.float32(1.0) if c >= 1 else c
    assert all(type(v) is np.float32 for v in (norm, c, coef)) and (coef == 1) == (sq == SQ_COEF_ONE)
    if coef == 1:  # a multiply by 1 or a round trip through fp32 would rewrite at least the signalling NaNs
        odd = torch.tensor(ODD_BITS[dt], dtype=PATTERN[dt][0])
        for t in [t for t in x if t.numel() >= 4][::3]:
            bits(t)[:2] = odd[:2]   # views: the patterns land in x
            bits(t)[-2:] = odd[2:]
        want = x
    else:
        want = [torch.from_numpy(t.float().numpy() * coef).to(dt) for t in x]
    out = GuardedList([3], F32, device)
    out.fill([torch.full((3,), 7.0)])

    def launch(plan):
        plan.set_clip(CLIP["max_norm"], CLIP["eps"], sqnorm=_scalar(device, float(sq32)), out=out.views[0])
        plan.clip_scale(0, dt)

    (got,) = run_guarded(device, numels, [(dt, x, off)], launch)
    (pub,) = _read_intact(out, "the published [sq, coef, norm]")
    assert same_bits(pub, torch.from_numpy(np.array([sq32, coef, norm], dtype=np.float32))), (pub, sq32, coef, norm)
    assert_lists(got, want, f"clip-scale by {coef}", nan_ok=False)


# ----------------------------------------------------- the policy children
def run_policy_suite(device):
    """What each child process of tests/test_gpu_pack_variants.py::test_policy_children runs under its
    environment setting: a fixed short list of the drivers above, on LIST_A and LIST_B."""
    for numels in (LIST_A, LIST_B):
        for align in (0, 64):
            for sd, fd, mode in ((F32, F32, "mul"), (F32, BF16, "div"), (BF16, BF16, "none"), (F16, F32, "none")):
                run_pack(device, numels, sd, fd, mode, align=align)
            run_unpack(device, numels, F32, F32, align=align, sqnorm=True)
            run_unpack(device, numels, BF16, F32, align=align, sqnorm=True)
            run_unpack_check(device, numels, BF16, F16, align=align)
        run_unpack_check(device, numels, BF16, F16, nonfinite=True)
        for dt in DTYPES:
            run_sqnorm_exact(device, numels, dt, 0)
            run_clip_scale(device, numels, dt, 0, SQ_CLIPS)
            run_clip_scale(device, numels, dt, 0, SQ_COEF_ONE)
