"""Shared by tests/test_seg_variants_cpu.py (host backend) and tests/test_gpu_seg_variants.py (the HIP
kernels): the LARS / LAMB half of the chunk engine — seg_sum_kernel with LarsLanes and LambLanes
(gs_lars_norms, gs_lamb_moments), lars_norm_finish, LarsOp and LambOp (gs_lars_step[_lowp],
gs_lamb_step[_lowp]) — against the numpy fp32 restatements of tests/_lars_common.py and
tests/_lamb_common.py, bit for bit, on guarded tensors.  Every driver takes a device, so one body
serves both backends.

No tolerance appears below (the one bound, in run_repeat_at_depth, is tests/_lars_common.py's
assert_sums_close, kept as a sanity check beside a bit comparison).  Every comparison is exact, and
may be, because
  * p, the momentum buffer, m, v and the low-precision copy are element-wise: the restatement, fed
    the per-tensor sums the library published, rounds every operation once as the contract
    (include/gsync.h) says, and the copy is one round-to-nearest-even cast of the stored fp32 p;
  * the per-tensor sums are compared on exact-sum inputs only: every square is a multiple of one
    power of two q and the sum of the squares is below 2^24 * q, so every fp32 partial sum, in any
    order, is exact.  assert_exact checks that on the CPU before anything is launched, together with
    what tests/_lamb_common.py::run_exact_step checks: the restatement's fp32 sums equal its fp64
    sums.  p is drawn from multiples of 0.5 in [-1, 1]; LARS's g from the same grid; with EXACT_HP
    LAMB's u is ±1 (+ 0.5 p on an adapted tensor);
  * where both sides hold a NaN any payload is accepted (same_bits_nan, through assert_lists);
    everywhere else it is bit equality.
Every tensor of every bound slot is guarded (tests/_update_common.py::GuardedList, through
run_guarded), the slots an op only reads included, and so is the published vector of sums.

Not reached: seg_sum_kernel's grid-stride loop (``g += gridDim.x``) needs more than 65536 groups of
4 chunks, over 2^28 elements — not a test of a few seconds.  It is a known, unreached path.
"""
import math

import numpy as np
import torch

from tests import _lamb_common as CL
from tests import _lars_common as CR
from tests._lars_common import SIZES2
from tests._update_common import (BF16, DT_IDS, DTYPES, F16, F32, LIST_A, LIST_B, LOWP_IDS, LOWPS,  # noqa: F401
                                  SPECIAL_NUMELS, GuardedList, _check_copy, _inputs, _scalar, _slot_offs, _sync,
                                  assert_lists, run_guarded, sentinel_list)

F = np.float32

# ------------------------------------------------------------- the chunk map
# build_chunk_map's rules (gs_plan.cpp, documented in tests/_lars_common.py): a tensor of >= 4 Ki
# elements starts on a multiple of 4 Ki, one of >= 1 Ki on a multiple of 1 Ki, any other on a
# multiple of 4; one descriptor per 1 Ki elements: (first tensor, 0 = full | span of a mixed chunk).
K_UNIT, K_CHUNK, K_GROUP, K_BLOCK = 4, 1024, 4096, 256


def chunk_map(numels):
    """(voff, [(t0, code)]) of a plan of ``numels``; (-1, -1) is an empty chunk"""
    n, voff, cur = len(numels), [], 0
    for m in numels:
        a = K_GROUP if m >= K_GROUP else (K_CHUNK if m >= K_CHUNK else K_UNIT)
        cur = -(-cur // a) * a
        voff.append(cur)
        cur += m
    chunks, t = [], 0
    for c in range(-(-cur // K_CHUNK)):
        lo, hi = c * K_CHUNK, (c + 1) * K_CHUNK
        while t < n and voff[t] + numels[t] <= lo:
            t += 1
        if t >= n or voff[t] >= hi:
            chunks.append((-1, -1))
            continue
        u = t
        while u < n and voff[u] < hi:
            u += 1
        full = voff[t] <= lo and voff[t] + numels[t] >= hi
        chunks.append((t, 0 if full else u - t))
    return voff, chunks


def slot_counts(numels):
    """partial slots per tensor: one per (chunk, tensor of its span) pair, as lars_prepare numbers them"""
    cnt = [0] * len(numels)
    for t0, code in chunk_map(numels)[1]:
        for i in range(1 if code == 0 else max(code, 0)):
            cnt[t0 + i] += 1
    return cnt


# a full group, a full chunk and a 3-element tail in one tensor, a second tensor of full chunks and
# a tail behind an alignment gap, and a tiny one: with one slot off 16 bytes all take the checked path
OFF_NUMELS = [4096 + 1024 + 3, 4099, 7]

# case F: one mixed chunk of 256 four-element tensors with an empty tensor in front of every fourth
# (the very first is skipped by the map: it ends where the chunk begins), a second mixed chunk of
# 1-3-element tensors, then a full chunk — all inside one group of 4 chunks
SPAN_LIST = [n for i in range(256) for n in (([0] if i % 4 == 0 else []) + [4])] + [1, 2, 3, 1] + [1024]
SPAN = 256 + 63


def assert_span_layout():
    """the span list still forms what it was built for; a layout change fails here, loudly"""
    _, chunks = chunk_map(SPAN_LIST)
    assert chunks == [(1, SPAN), (SPAN + 1, 4), (SPAN + 5, 0)], chunks
    assert SPAN >= 300 > K_BLOCK
    cnt = slot_counts(SPAN_LIST)
    assert cnt[0] == 0 and all(c == 1 for c in cnt[1:])  # the empties inside the run own a slot too


# case G: tensors of 255 ... 2049 partial slots (ragged last chunks), small ones between them
FOLD_SLOTS = [255, 256, 257, 1023, 1024, 1025, 2049]
FOLD_LIST = []
for _k in FOLD_SLOTS:
    FOLD_LIST += [7, 3, (_k - 1) * 1024 + 1 + (_k * 37) % 1000]
FOLD_LIST += [5]
FOLD_BIG = [3 * i + 2 for i in range(len(FOLD_SLOTS))]


def assert_fold_layout():
    cnt = slot_counts(FOLD_LIST)
    assert [cnt[t] for t in FOLD_BIG] == FOLD_SLOTS, cnt
    assert sum(FOLD_LIST) < 6.2e6 and max(FOLD_LIST) < 2 ** 22


LISTS = {"listA": LIST_A, "listB": LIST_B, "sizes2": SIZES2, "span": SPAN_LIST}


# ------------------------------------------------------------------ helpers
def _np(ts):
    return [t.float().numpy().copy() for t in ts]


def _t(arrs):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in arrs]


def _alt(n, first=True):
    return [(i % 2 == 0) == first for i in range(n)]


class Norms:
    """the published fp32[2n], guarded, pre-filled with the sentinel: every entry must be written"""

    def __init__(self, device, n):
        self.device, self.n = device, n
        self.gl = GuardedList([2 * n], F32, device)
        self.gl.fill(None)
        self.t = self.gl.views[0]

    def read(self, written=True):
        _sync(self.device)
        (vals,), intact = self.gl.read()
        assert intact, "a guard element around the per-tensor sums changed"
        a = vals.numpy().copy()
        if written:  # the sentinel is a NaN with a payload no sum of squares produces
            assert not (a.view(np.int32) == 0x7FC00001).any(), "a per-tensor sum was not written"
        return a


def assert_exact(sq_terms, sums32, what):
    """``sq_terms``: per tensor, the values whose squares are summed.  Every square is a multiple
    of one power of two q and their sum is below 2^24 q — any fp32 partial sum, in any order, is
    exact — and the restatement's fp32 sums equal the fp64 ones."""
    for t, x in enumerate(sq_terms):
        sq = x.astype(np.float64) ** 2
        q = next((q for q in (1.0, 0.25, 0.0625) if not np.any(np.mod(sq, q))), None)
        assert q is not None, f"{what}: tensor {t}: a square off the 1/16 grid"
        total = float(sq.sum())
        assert total / q < 2 ** 24, f"{what}: tensor {t}: sum {total} not exact in fp32 (q = {q})"
        assert float(sums32[t]) == total, f"{what}: tensor {t}: the fp32 restatement is not exact"


def assert_sums_bits(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    assert bad.size == 0, f"{what}: sums differ at {bad[:8]}: {got[bad[:8]]} != {want[bad[:8]]}"


def assert_sums_class(got, want, what):
    """random inputs: the sums are order-dependent, but whether one is NaN or infinite is not
    (squares are >= 0 or NaN, and the finite inputs are far from overflow)"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN sums differ"
    assert np.array_equal(np.isinf(got), np.isinf(want)), f"{what}: infinite sums differ"
    assert not np.signbit(got[~np.isnan(got)]).any(), f"{what}: a negative sum"


def _grid(n, gen, lo=-2, hi=2):
    """multiples of 0.5 in [lo / 2, hi / 2]"""
    return torch.randint(lo, hi + 1, (n,), generator=gen).float() * 0.5


def _nonzero_grid(n, gen):
    """non-zero multiples of 0.5 in [-2, 2]"""
    x = torch.randint(1, 5, (n,), generator=gen).float() * 0.5
    return x * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)


def exact_inputs(numels, gdt, seed, lamb, ends=False):
    """exact-sum (p, g, m or buf, v).  LARS: p, g on the 0.5 grid in [-1, 1], a random buffer.
    LAMB: g non-zero on the 0.5 grid in [-2, 2], m = v = 0.  ``ends``: the first and the last
    element of every tensor are non-zero."""
    gen = torch.Generator().manual_seed(seed)
    p = [_grid(n, gen) for n in numels]
    g = [(_nonzero_grid(n, gen) if lamb else _grid(n, gen)) for n in numels]
    if ends:
        for x in p + g:
            if x.numel():
                x[0] = 0.5 if x[0] == 0 else x[0]
                x[-1] = -1.0 if x[-1] == 0 else x[-1]
    g = [x.to(gdt) for x in g]
    if lamb:
        m, v = [torch.zeros(n) for n in numels], [torch.zeros(n) for n in numels]
    else:
        m, v = [torch.randn(n, generator=gen) for n in numels], None
    return p, g, m, v


def sparse_inputs(numels, gdt, seed, lamb):
    """case G's second variant: chunk k of a tensor holds one non-zero p, 2^(k mod 6), at a place
    that moves with k (and for LARS one non-zero g, 2^((k + 3) mod 6)): every partial slot
    contributes a different power of 4 than its neighbours, so a swapped, doubled or dropped slot
    changes the sum.  (k mod 12, powers of 4 up to 4^11, would pass 2^24 over 2049 slots.)  LAMB's g
    stays non-zero everywhere — u = ±1 + 0.5 p on these adapted tensors."""
    gen = torch.Generator().manual_seed(seed)
    p = [torch.zeros(n) for n in numels]
    g = [(_nonzero_grid(n, gen) if lamb else torch.zeros(n)) for n in numels]
    for t, n in enumerate(numels):
        for k in range(-(-n // K_CHUNK)):
            size = min(K_CHUNK, n - k * K_CHUNK)
            p[t][k * K_CHUNK + (k * 97) % size] = 2.0 ** (k % 6)
            if not lamb:
                g[t][k * K_CHUNK + (k * 61 + 5) % size] = -(2.0 ** ((k + 3) % 6))
    g = [x.to(gdt) for x in g]
    m, v = [torch.zeros(n) for n in numels], ([torch.zeros(n) for n in numels] if lamb else None)
    return p, g, m, v


def random_inputs(numels, gdt, seed, special=False, zero_p=(), zero_g=()):
    """tests/_update_common.py's random inputs (a few decades; m doubles as LARS's buffer), with
    all-zero p on the tensors of ``zero_p`` and all-zero g, m, v on those of ``zero_g``"""
    p, g, m, v = ([x.clone() for x in xs] for xs in _inputs(tuple(numels), gdt, seed, special))
    for t in zero_p:
        p[t].zero_()
    for t in zero_g:
        for xs in (g, m, v):
            xs[t].zero_()
    return p, g, m, v


# LIST_A with two 300-element tensors behind it: an all-zero p and an all-zero g (m, v), both adapted
LIST_C = LIST_A + [300, 300]
C_ZERO_P, C_ZERO_G = len(LIST_C) - 2, len(LIST_C) - 1
ADAPT_C = _alt(len(LIST_C))
ADAPT_C[C_ZERO_P] = ADAPT_C[C_ZERO_G] = True


# --------------------------------------------------------- A. gs_lars_norms
def run_lars_norms(device, numels, gdt, p_off, g_off, inputs=None, seed=61):
    """gs_lars_norms on exact-sum inputs: Σp², Σg² bit for bit (an empty tensor publishes +0), p
    and g unchanged, no guard moved"""
    numels = tuple(numels)
    p, g, _, _ = inputs or exact_inputs(numels, gdt, seed, lamb=False)
    rp, rg = _np(p), _np(g)
    want = CR.ref_sums(rp, rg)
    assert_exact(rp, want[0::2], "Σp²")
    assert_exact(rg, want[1::2], "Σg²")
    norms = Norms(device, len(numels))
    got_p, got_g = run_guarded(device, numels, [(F32, p, p_off), (gdt, g, g_off)],
                               lambda plan: plan.lars_norms(gdt, norms.t))
    assert_sums_bits(norms.read(), want, "gs_lars_norms")
    assert_lists(got_p, p, "p (read-only)", nan_ok=False)
    assert_lists(got_g, g, "grads (read-only)", nan_ok=False)


# ------------------------------------------------------------------- LAMB
RANDOM_HP = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-6, wd=0.01, bias_correction=True)


def _lamb_once(device, numels, gdt, ldt, inputs, offs, adapt, hp, step, grad_scale=None, found_inf=None, lo=0.0,
               hi=math.inf, do_step=True, unbind_g=False, hyper=None, again=None, null=False):
    """gs_lamb_moments (and gs_lamb_step[_lowp]) on guarded tensors; returns (what the slots hold,
    the published sums per moments call).  ``hyper`` = wrong host arguments dict: the true values go
    into a hyper source.  ``again``: clear the source and run the step a second time."""
    p, g, m, v = inputs
    n = len(numels)
    slots = [(F32, p, offs[0]), (gdt, g, offs[1]), (F32, m, offs[2]), (F32, v, offs[3])]
    if ldt is not None and do_step:
        slots.append((ldt, None, offs[4]))
    norms, sums = Norms(device, n), []
    bc1, bc2s = CL.bias_corrections(*hp["betas"], step, hp["bias_correction"])

    def step_once(plan, lr, c1, c2):
        gs = None if grad_scale is None else _scalar(device, grad_scale)
        fi = None if found_inf is None else _scalar(device, found_inf)
        plan.lamb_moments(gdt, *hp["betas"], hp["eps"], hp["wd"], c1, c2, norms.t, grad_scale=gs, found_inf=fi)
        sums.append(norms.read(written=not found_inf))
        if do_step:
            if unbind_g:  # the update pass reads slots 0, 2, 3 alone: slot 1 may be unbound
                plan.set_ptrs(1, [None] * n)
            plan.lamb(lr, hp["eps"], hp["wd"], c1, c2, norms.t, lo, hi, found_inf=fi, lowp_dtype=ldt)

    def launch(plan):
        plan.set_adapt(adapt)
        if null:  # NULL pointers on the (all empty) tensors
            for s in range(len(slots)):
                plan.set_ptrs(s, [None] * n)
        if hyper is not None:  # the source holds the true values; the arguments are deliberately wrong
            plan.set_hyper_source(torch.tensor([hp["lr"], bc1, bc2s], dtype=torch.float32, device=device))
            step_once(plan, hyper["lr"], hyper["bc1"], hyper["bc2s"])
            if again:
                plan.set_hyper_source(None)
                step_once(plan, hyper["lr"], hyper["bc1"], hyper["bc2s"])
        else:
            step_once(plan, hp["lr"], bc1, bc2s)

    return run_guarded(device, numels, slots, launch), sums


def _lamb_ref(inputs, adapt, hp, step, sums, grad_scale, lo, hi):
    rp, rg, rm, rv = (_np(x) for x in inputs)
    with np.errstate(all="ignore"):
        return CL.ref_plan_step(rp, rg, rm, rv, adapt, hp, step, sums=sums, mult=grad_scale, lo=lo, hi=hi)


def run_lamb_exact(device, numels, gdt, off_slot=None, grad_scale=None, adapt=None, inputs=None, ldt=None,
                   do_step=False, seed=62):
    """gs_lamb_moments on exact-sum inputs with EXACT_HP: Σp², Σu², m' and v' bit for bit against
    the restatement's own sums; p and g unchanged (or, with ``do_step``, p and the copy after
    gs_lamb_step[_lowp], bit for bit)"""
    numels = tuple(numels)
    adapt = _alt(len(numels)) if adapt is None else adapt
    inputs = inputs or exact_inputs(numels, gdt, seed, lamb=True)
    wp, wm, wv, u, want = _lamb_ref(inputs, adapt, CL.EXACT_HP, 1, None, grad_scale, 0.0, math.inf)
    assert_exact(_np(inputs[0]), want[0::2], "Σp²")
    assert_exact(u, want[1::2], "Σu²")
    got, sums = _lamb_once(device, numels, gdt, ldt, inputs, _slot_offs(5, off_slot), adapt, CL.EXACT_HP, 1,
                           grad_scale=grad_scale, do_step=do_step)
    assert_sums_bits(sums[0], want, "gs_lamb_moments")
    assert_lists(got[2], _t(wm), "m'")
    assert_lists(got[3], _t(wv), "v'")
    assert_lists(got[1], inputs[1], "grads (read-only)", nan_ok=False)
    if do_step:
        assert_lists(got[0], _t(wp), "p")
        if ldt is not None:
            _check_copy(got[0], got[4], ldt)
    else:
        assert_lists(got[0], inputs[0], "p (read-only)", nan_ok=False)


def run_lamb(device, numels, gdt, ldt=None, off_slot=None, grad_scale=None, adapt=None, hp=RANDOM_HP, lo=0.0,
             hi=math.inf, do_step=True, unbind_g=True, inputs=None, special=False, zero_p=(), zero_g=(),
             clamped=None, hyper=False, seed=24):
    """One LAMB step on random inputs: m', v' bit for bit; p and the copy bit for bit against the
    restatement fed the published sums; the grads untouched; the copy the cast of the stored p.
    ``clamped`` = "lo" / "hi": some adapted tensor's free ratio lies outside the clamp on that side.
    ``hyper``: the true [lr, bc1, bc2s] come from a hyper source while the host arguments are
    wrong; then the source is cleared and a second step follows the host arguments."""
    numels = tuple(numels)
    n = len(numels)
    adapt = _alt(n) if adapt is None else adapt
    inputs = inputs or random_inputs(numels, gdt, seed, special, zero_p, zero_g)
    wrong = dict(lr=0.5, bc1=0.75, bc2s=0.25) if hyper else None
    got, sums = _lamb_once(device, numels, gdt, ldt, inputs, _slot_offs(5, off_slot), adapt, hp, 3,
                           grad_scale=grad_scale, lo=lo, hi=hi, do_step=do_step, unbind_g=unbind_g and not hyper,
                           hyper=wrong, again=hyper)
    wp, wm, wv, u, _ = _lamb_ref(inputs, adapt, hp, 3, sums[0], grad_scale, lo, hi)
    with np.errstate(all="ignore"):
        assert_sums_class(sums[0], CL.ref_sums(_np(inputs[0]), u), "gs_lamb_moments")
    if hyper:  # the second step: the host arguments, as bias corrections of "step" and lr
        nm, nv, _ = CL.ref_moments(wp, _np(inputs[1]), wm, wv, adapt, *hp["betas"], hp["eps"], hp["wd"], wrong["bc1"],
                                   wrong["bc2s"], grad_scale)
        wp = CL.ref_update(wp, nm, nv, sums[1], adapt, wrong["lr"], hp["eps"], hp["wd"], wrong["bc1"], wrong["bc2s"],
                           lo, hi)
        wm, wv = nm, nv
    for t in zero_p:  # ratio 1: ‖p‖ = 0
        assert adapt[t] and sums[0][2 * t] == 0
    for t in zero_g:  # u is the decay term alone; without a decay ‖u‖ = 0 and the ratio is 1
        assert adapt[t] and (hp["wd"] != 0 or sums[0][2 * t + 1] == 0)
    if clamped is not None:
        free = CL.ref_ratios(sums[0], adapt)
        live = [t for t in range(n) if adapt[t] and sums[0][2 * t] > 0 and sums[0][2 * t + 1] > 0]
        assert any(free[t] < F(lo) for t in live) if clamped == "lo" else any(free[t] > F(hi) for t in live)
    assert_lists(got[2], _t(wm), "m'")
    assert_lists(got[3], _t(wv), "v'")
    assert_lists(got[1], inputs[1], "grads (read-only)", nan_ok=False)
    if do_step:
        assert_lists(got[0], _t(wp), "p")
        if ldt is not None:
            assert_lists(got[4], [x.to(ldt) for x in _t(wp)], "copy")
            _check_copy(got[0], got[4], ldt)
    else:
        assert_lists(got[0], inputs[0], "p (read-only)", nan_ok=False)


def run_lamb_found_inf(device, numels, gdt, ldt, off_slot=None):
    """found_inf = 1: p, g, m, v keep their bits, the copy keeps the sentinel, no guard moves.  The
    sums are unspecified for a skipped step (include/gsync.h): only their guards are checked."""
    numels = tuple(numels)
    inputs = random_inputs(numels, gdt, 25)
    got, _ = _lamb_once(device, numels, gdt, ldt, inputs, _slot_offs(5, off_slot), _alt(len(numels)), RANDOM_HP, 3,
                        grad_scale=0.37, found_inf=1.0)
    for k, name in enumerate(("p", "grads", "m", "v")):
        assert_lists(got[k], inputs[k], f"found_inf: {name}", nan_ok=False)
    if ldt is not None:
        assert_lists(got[4], sentinel_list(numels, ldt), "found_inf: copy", nan_ok=False)


def lamb_special_inputs(numels, gdt, seed=26):
    """random inputs with every special value at a tensor's first and at a tensor's last element of g
    (tests/_update_common.py::_place_specials; "zero_v0" also has v = 0 there) and g = m = v = 0 at the
    last element of the 65-element tensor, inside a mixed chunk (that spot repeats a special value
    other edges already hold), and at the last element of the 4097-element tensor's full chunks: with
    eps = 0 that one element's u is 0/0"""
    p, g, m, v = random_inputs(numels, gdt, seed, special=True)
    for n, i in ((65, 64), (4097, 4095)):
        t = list(numels).index(n)
        g[t][i], m[t][i], v[t][i] = 0.0, 0.0, 0.0
    return p, g, m, v


# ------------------------------------------------------------------- LARS
LARS_HP = dict(lr=0.1, eta=1e-3, eps=1e-8)


def _lars_once(device, numels, gdt, ldt, inputs, offs, adapt, mom, wd, grad_scale=None, found_inf=None,
               fresh_norms=False, hyper=None, again=False, null=False):
    """gs_lars_norms and gs_lars_step[_lowp] on guarded tensors; returns (what the slots hold, the
    published sums).  ``fresh_norms``: the sums come from another plan over the same values, so this
    plan's step has seen no gs_lars_norms and loads its grads non-temporally (NTG = true); else the
    step runs right behind this plan's own gs_lars_norms (NTG = false)."""
    p, g, b = inputs[:3]
    n = len(numels)
    slots = [(F32, p, offs[0]), (gdt, g, offs[1]), (F32, b if mom != 0 else None, offs[2])]
    if ldt is not None:
        slots.append((ldt, None, offs[3]))
    norms, sums = Norms(device, n), []

    def step_once(plan, lr):
        gs = None if grad_scale is None else _scalar(device, grad_scale)
        fi = None if found_inf is None else _scalar(device, found_inf)
        if fresh_norms:
            assert not sums, "a second step takes this plan's own gs_lars_norms"
            run_guarded(device, numels, [(F32, p, 0), (gdt, g, 0)], lambda q: q.lars_norms(gdt, norms.t))
        else:
            plan.lars_norms(gdt, norms.t)
        sums.append(norms.read())
        plan.lars(gdt, lr, mom, wd, LARS_HP["eta"], LARS_HP["eps"], norms.t, grad_scale=gs, found_inf=fi,
                  lowp_dtype=ldt)

    def launch(plan):
        plan.set_adapt(adapt)
        if mom == 0:  # without a momentum slot 2 is unbound
            plan.set_ptrs(2, [None] * n)
        if null:
            for s in range(len(slots)):
                plan.set_ptrs(s, [None] * n)
        if hyper is not None:  # the source holds the true lr; the argument is deliberately wrong
            plan.set_hyper_source(torch.tensor([LARS_HP["lr"], 0.0, 0.0], dtype=torch.float32, device=device))
            step_once(plan, hyper)
            if again:
                plan.set_hyper_source(None)
                step_once(plan, hyper)
        else:
            step_once(plan, LARS_HP["lr"])

    return run_guarded(device, numels, slots, launch), sums


def _lars_ref(inputs, sums, adapt, lr, mom, wd, grad_scale):
    rp, rg, rb = (_np(x) for x in inputs[:3])
    with np.errstate(all="ignore"):
        return CR.ref_step(rp, rg, rb, sums, adapt, lr, mom, wd, LARS_HP["eta"], LARS_HP["eps"], grad_scale)


def run_lars(device, numels, gdt, ldt=None, off_slot=None, mom=0.9, wd=1e-4, grad_scale=None, adapt=None,
             found_inf=None, inputs=None, special=False, zero_p=(), zero_g=(), arms=(False, True), exact=False,
             seed=23):
    """One LARS step, both arms of the grad load (``arms``: False = right behind this plan's
    gs_lars_norms, NTG = false; True = a fresh plan handed another plan's sums, NTG = true): p, the
    buffer and the copy bit for bit against the restatement fed the published sums, and the two arms
    against each other, sums included; the grads untouched; without a momentum slot 2 is unbound and
    its tensors keep the sentinel.  ``found_inf`` = 1: nothing is written.  ``exact``: exact-sum
    inputs, and the published sums equal the restatement's own."""
    numels = tuple(numels)
    n = len(numels)
    adapt = _alt(n) if adapt is None else adapt
    if inputs is None:
        inputs = exact_inputs(numels, gdt, seed, lamb=False) if exact else \
            random_inputs(numels, gdt, seed, special, zero_p, zero_g)
    p, g, b = inputs[:3]
    offs = _slot_offs(4, off_slot)
    runs = [_lars_once(device, numels, gdt, ldt, inputs, offs, adapt, mom, wd, grad_scale, found_inf, fresh)
            for fresh in arms]
    with np.errstate(all="ignore"):
        own = CR.ref_sums(_np(p), _np(g))
    if exact:
        assert_exact(_np(p), own[0::2], "Σp²")
        assert_exact(_np(g), own[1::2], "Σg²")
    sentinel = sentinel_list(numels, F32)
    for got, sums in runs:
        (assert_sums_bits if exact else assert_sums_class)(sums[0], own, "gs_lars_norms")
        for t in zero_p:
            assert adapt[t] and sums[0][2 * t] == 0
        for t in zero_g:
            assert adapt[t] and sums[0][2 * t + 1] == 0
        assert_lists(got[1], g, "grads (read-only)", nan_ok=False)
        if found_inf:
            assert_lists(got[0], p, "found_inf: p", nan_ok=False)
            assert_lists(got[2], b if mom != 0 else sentinel, "found_inf: buffer", nan_ok=False)
            if ldt is not None:
                assert_lists(got[3], sentinel_list(numels, ldt), "found_inf: copy", nan_ok=False)
            continue
        wp, wb = _lars_ref(inputs, sums[0], adapt, LARS_HP["lr"], mom, wd, grad_scale)
        assert_lists(got[0], _t(wp), "p")
        if mom != 0:
            assert_lists(got[2], _t(wb), "momentum buffer")
        else:
            assert_lists(got[2], sentinel, "momentum buffer (unbound)", nan_ok=False)
        if ldt is not None:
            assert_lists(got[3], [x.to(ldt) for x in _t(wp)], "copy")
            _check_copy(got[0], got[3], ldt)
    if len(runs) == 2:
        assert_sums_bits(runs[0][1][0], runs[1][1][0], "sums of the two plans")
        for s in range(len(runs[0][0])):
            assert_lists(runs[0][0][s], runs[1][0][s], f"cached-load arm vs non-temporal arm, slot {s}")


def run_lars_hyper(device, numels, gdt, ldt):
    """Eager hyper source: lr from a device [lr, -, -] while the host argument is wrong — bit-equal
    to the restatement at the device value; then the source is cleared and a second step follows the
    host argument."""
    numels = tuple(numels)
    adapt = _alt(len(numels))
    inputs = random_inputs(numels, gdt, 27)
    mom, wd, wrong = 0.9, 1e-4, 0.7
    got, sums = _lars_once(device, numels, gdt, ldt, inputs, _slot_offs(4, None), adapt, mom, wd, hyper=wrong,
                           again=True)
    p1, b1 = _lars_ref(inputs, sums[0], adapt, LARS_HP["lr"], mom, wd, None)
    with np.errstate(all="ignore"):
        p2, b2 = CR.ref_step(p1, _np(inputs[1]), b1, sums[1], adapt, wrong, mom, wd, LARS_HP["eta"], LARS_HP["eps"])
    assert_lists(got[0], _t(p2), "p after the source was cleared")
    assert_lists(got[2], _t(b2), "momentum buffer after the source was cleared")
    if ldt is not None:
        _check_copy(got[0], got[3], ldt)
    # the first step alone, against the restatement at the device value
    got, sums = _lars_once(device, numels, gdt, ldt, inputs, _slot_offs(4, None), adapt, mom, wd, hyper=wrong)
    p1, b1 = _lars_ref(inputs, sums[0], adapt, LARS_HP["lr"], mom, wd, None)
    assert_lists(got[0], _t(p1), "p from the hyper source")
    assert_lists(got[2], _t(b1), "momentum buffer from the hyper source")


def run_lamb_hyper(device, numels, gdt, ldt):
    """LAMB's counterpart: [lr, bc1, bc2s] from the source, read by both passes"""
    numels = tuple(numels)
    inputs = random_inputs(numels, gdt, 28)
    # the first step alone, against the restatement at the device values
    got, sums = _lamb_once(device, numels, gdt, ldt, inputs, _slot_offs(5, None), _alt(len(numels)), RANDOM_HP, 3,
                           hyper=dict(lr=0.5, bc1=0.75, bc2s=0.25))
    wp, wm, wv, _, _ = _lamb_ref(inputs, _alt(len(numels)), RANDOM_HP, 3, sums[0], None, 0.0, math.inf)
    assert_lists(got[0], _t(wp), "p from the hyper source")
    assert_lists(got[2], _t(wm), "m' from the hyper source")
    assert_lists(got[3], _t(wv), "v' from the hyper source")
    run_lamb(device, numels, gdt, ldt, inputs=inputs, hyper=True)


# ------------------------------------------------------- G, J. fold depth
def run_fold_lars(device, gdt, sparse):
    assert_fold_layout()
    numels = tuple(FOLD_LIST)
    inputs = sparse_inputs(numels, gdt, 63, lamb=False) if sparse else \
        exact_inputs(numels, gdt, 63, lamb=False, ends=True)
    run_lars_norms(device, numels, gdt, 0, 0, inputs=inputs)


def run_fold_lamb(device, gdt, sparse):
    """the large tensors unadapted on the grid inputs (u = ±1, Σu² = numel), adapted on the sparse
    ones (u = ±1 + 0.5 p: one element per chunk differs, by a power of two that moves with the chunk)"""
    assert_fold_layout()
    numels = tuple(FOLD_LIST)
    if sparse:
        inputs, adapt = sparse_inputs(numels, gdt, 64, lamb=True), [True] * len(numels)
    else:
        inputs = exact_inputs(numels, gdt, 64, lamb=True, ends=True)
        adapt = [t not in FOLD_BIG and t % 2 == 0 for t in range(len(numels))]
    run_lamb_exact(device, numels, gdt, adapt=adapt, inputs=inputs)


def run_repeat_at_depth(device, gdt=F32):
    """The plan of case G twice, on fresh plans, on random inputs: Σp², Σu² bit-identical between
    the runs ("replicas publish the same bits", at slot counts where the fold loops) and, as a
    sanity check only, inside tests/_lars_common.py's numel * 2^-23 bound."""
    assert_fold_layout()
    numels = tuple(FOLD_LIST)
    gen = torch.Generator().manual_seed(65)
    inputs = tuple([f(torch.randn(n, generator=gen)) for n in numels]
                   for f in (lambda x: x, lambda x: x.to(gdt), lambda x: x, lambda x: x * x))
    adapt = _alt(len(numels))
    runs = [_lamb_once(device, numels, gdt, None, inputs, _slot_offs(5, None), adapt, RANDOM_HP, 3, do_step=False)
            for _ in range(2)]
    assert_sums_bits(runs[0][1][0], runs[1][1][0], "two fresh plans")
    for s in (2, 3):
        assert_lists(runs[0][0][s], runs[1][0][s], f"two fresh plans, slot {s}", nan_ok=False)
    _, wm, wv, u, _ = _lamb_ref(inputs, adapt, RANDOM_HP, 3, runs[0][1][0], None, 0.0, math.inf)
    assert_lists(runs[0][0][2], _t(wm), "m'")
    assert_lists(runs[0][0][3], _t(wv), "v'")
    CR.assert_sums_close(runs[0][1][0], _np(inputs[0]), u)


# ---------------------------------------------------- H. degenerate plans
def run_degenerate(device, numels, gdt=F32, ldt=BF16):
    """Both passes of both optimizers on a plan of ``numels`` — none, empty ones (with NULL
    pointers), one element, exactly one full group, one group and one element: every call returns 0
    (TensorListPlan raises otherwise), the sums are exact (0 where there are no elements), every
    tensor matches the restatement and nothing outside the tensors is written."""
    numels = tuple(numels)
    null = len(numels) > 0 and not any(numels)
    n = len(numels)
    adapt = [True] * n
    inputs = exact_inputs(numels, gdt, 66, lamb=False)
    got, sums = _lars_once(device, numels, gdt, ldt, inputs, _slot_offs(4, None), adapt, 0.9, 1e-4, null=null)
    own = CR.ref_sums(_np(inputs[0]), _np(inputs[1]))
    assert_exact(_np(inputs[0]), own[0::2], "Σp²")
    assert_exact(_np(inputs[1]), own[1::2], "Σg²")
    assert_sums_bits(sums[0], own, "gs_lars_norms")
    wp, wb = _lars_ref(inputs, sums[0], adapt, LARS_HP["lr"], 0.9, 1e-4, None)
    assert_lists(got[0], _t(wp), "LARS p")
    assert_lists(got[2], _t(wb), "LARS momentum buffer")
    _check_copy(got[0], got[3], ldt)
    inputs = exact_inputs(numels, gdt, 67, lamb=True)
    got, sums = _lamb_once(device, numels, gdt, ldt, inputs, _slot_offs(5, None), adapt, CL.EXACT_HP, 1, null=null)
    wp, wm, wv, u, want = _lamb_ref(inputs, adapt, CL.EXACT_HP, 1, None, None, 0.0, math.inf)
    assert_exact(_np(inputs[0]), want[0::2], "Σp²")
    assert_exact(u, want[1::2], "Σu²")
    assert_sums_bits(sums[0], want, "gs_lamb_moments")
    assert_lists(got[0], _t(wp), "LAMB p")
    assert_lists(got[2], _t(wm), "LAMB m'")
    assert_lists(got[3], _t(wv), "LAMB v'")
    _check_copy(got[0], got[4], ldt)
    if not any(numels):
        assert not sums[0].view(np.int32).any(), "sums of a plan without elements must be +0"
