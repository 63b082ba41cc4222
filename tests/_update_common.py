"""Shared by tests/test_update_variants_cpu.py (host backend) and tests/test_gpu_update_variants.py
(the HIP kernels): the oldest ops of the chunk engine — SgdOp, AdamOp, ScaleOp, SumOp, UnscaleOp —
against a plain reference, bit for bit, on guarded tensors.  Every driver takes a device, so one
body serves both backends.

No tolerance appears below.  Every comparison is exact, and may be, because
  * the oracle (oracle/gs_oracle.c, or_sgd / or_adam) restates the kernels' fp32 expression op for
    op — the same fmaf calls, compiled without contraction — so SGD and Adam agree in every bit;
  * every 16-bit store (the low-precision copy, the 16-bit scale and unscale) is one
    round-to-nearest-even cast of the value the kernel STORED in fp32: ``p.to(ldt)`` in torch,
    O.f32_to_bf16 in numpy;
  * gs_scale and gs_unscale_check are one IEEE multiply or divide in fp32 and that cast, which
    numpy and torch's CPU kernel compute the same way;
  * gs_sum's inputs are integers in [-8, 8] with 16 * numel < 2^24: every fp32 partial sum, in any
    order, is an integer below 2^24 and so exact — twice over, for the accumulating launch.
Where both sides hold a NaN the comparison accepts any payload (same_bits_nan); everywhere else,
and wherever a test pins a NaN pattern itself, it is bit equality.
"""
import functools
import math

import numpy as np
import torch

from oracle import oracle as O
from tests._ema_common import LIST_A, LIST_B, bits, same_bits  # noqa: F401  (re-exported)

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
DT_IDS = ["f32", "bf16", "f16"]
LOWPS = [None, BF16, F16]
LOWP_IDS = ["none", "bf16", "f16"]
LOWP_NAME = {None: None, BF16: "bf16", F16: "f16"}

# a last group shorter than the op's group (Adam: 4 chunks of 1 Ki elements, SGD: 2)
GROUPS_ADAM = [[3 * 1024], [5 * 1024 + 1], [1024]]
GROUPS_SGD = GROUPS_ADAM + [[1024 + 1]]
GROUP_IDS = ["3Ki", "5Ki+1", "1Ki", "1Ki+1"]
OFF_SLOT_NUMELS = [4099]  # full groups, one full chunk and a 3-element tail, all on the checked path

G = 16  # guard elements on each side of every tensor
# NaN payloads: a kernel that reads a guard poisons its result, one that writes it changes the pattern
PATTERN = {F32: (torch.int32, 0x7FC00001), BF16: (torch.int16, 0x7FC1), F16: (torch.int16, 0x7E01)}


def same_bits_nan(x, y):
    """bit-equal, except that two NaNs at the same place compare equal whatever their payloads"""
    x, y = x.cpu(), y.cpu()
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    nx, ny = torch.isnan(x), torch.isnan(y)
    return torch.equal(nx, ny) and torch.equal(bits(x)[~nx], bits(y)[~ny])


def assert_lists(got, want, what, nan_ok=True):
    assert len(got) == len(want), what
    eq = same_bits_nan if nan_ok else same_bits
    for t, (a, r) in enumerate(zip(got, want)):
        assert eq(a, r), f"{what}: tensor {t} ({a.numel()} elements) differs"


class GuardedList:
    """One plan slot's tensors.  Tensor t is the slice ``backing[G+off : G+off+n]`` of its own
    backing buffer; everything outside the slice holds the dtype's sentinel.  ``off = 0`` keeps the
    slice 16-byte aligned (the vector path), ``off = 1`` puts it one element off (the checked path).
    ``offs`` may also be a list, one per tensor."""

    def __init__(self, numels, dtype, device, off=0):
        self.numels, self.dtype, self.device = list(numels), dtype, device
        self.itype, self.pat = PATTERN[dtype]
        self.offs = list(off) if isinstance(off, (list, tuple)) else [off] * len(self.numels)
        self.sizes = [G + o + n + G for n, o in zip(self.numels, self.offs)]
        self.raw = [torch.empty(s, dtype=self.itype, device=device) for s in self.sizes]
        self.views = [r.view(dtype)[G + o:G + o + n] for r, n, o in zip(self.raw, self.numels, self.offs)]
        for r, v, o in zip(self.raw, self.views, self.offs):
            assert r.data_ptr() % 16 == 0 and (v.numel() == 0 or (v.data_ptr() % 16 == 0) == (o == 0))
        mask = torch.ones(sum(self.sizes), dtype=torch.bool)
        pos = 0
        for s, n, o in zip(self.sizes, self.numels, self.offs):
            mask[pos + G + o:pos + G + o + n] = False
            pos += s
        self.guard_mask = mask

    def fill(self, values=None):
        """values: CPU tensors of the slot's dtype; None leaves the sentinel in the tensors too"""
        host = torch.full((sum(self.sizes),), self.pat, dtype=self.itype)
        if values is not None:
            pos = 0
            for s, n, o, x in zip(self.sizes, self.numels, self.offs, values):
                assert x.dtype == self.dtype and x.numel() == n
                host[pos + G + o:pos + G + o + n] = bits(x)
                pos += s
        for r, h in zip(self.raw, host.to(self.device).split(self.sizes)):
            r.copy_(h)

    def read(self):
        """(the tensors on the CPU, whether every guard element still holds the sentinel)"""
        if not self.raw:
            return [], True
        host = torch.cat(self.raw).cpu()
        intact = bool((host[self.guard_mask] == self.pat).all())
        out = [h[G + o:G + o + n].clone().view(self.dtype)
               for h, n, o in zip(host.split(self.sizes), self.numels, self.offs)]
        return out, intact


def sentinel_list(numels, dtype):
    """what :meth:`GuardedList.read` returns for a slot nobody wrote since ``fill(None)``"""
    itype, pat = PATTERN[dtype]
    return [torch.full((n,), pat, dtype=itype).view(dtype) for n in numels]


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def run_guarded(device, numels, slots, launch):
    """Bind ``slots`` — [(dtype, CPU values or None, off)] for plan slots 0, 1, ... — as guarded
    tensors, call ``launch(plan)``, assert after it that no guard changed, and return what each
    slot holds.  The helper every test of this module goes through."""
    from distributed_training_amd.multi_tensor import TensorListPlan, update_task_units

    lists = []
    for dtype, values, off in slots:
        gl = GuardedList(numels, dtype, device, off)
        gl.fill(values)
        lists.append(gl)
    plan = TensorListPlan(numels, device, task_units=update_task_units(device))
    try:
        for s, gl in enumerate(lists):
            plan.set_ptrs(s, gl.views)
        launch(plan)
        _sync(device)
    finally:
        plan.close()
    out = []
    for s, gl in enumerate(lists):
        values, intact = gl.read()
        assert intact, f"slot {s}: a guard element around a tensor changed"
        out.append(values)
    return out


def _scalar(device, x):
    return torch.tensor([x], dtype=torch.float32, device=device)


def _slot_offs(n_slots, off_slot):
    offs = [0] * n_slots
    if off_slot is not None:
        offs[off_slot] = 1
    return offs


# ------------------------------------------------------------------ inputs
def _to_np(x):
    """the oracle's view of a CPU tensor: float32, bf16 bit patterns (uint16) or float16"""
    if x.dtype == BF16:
        return bits(x).numpy().view(np.uint16)
    return x.contiguous().numpy()


def _from_lowp(a, ldt):
    if ldt == BF16:
        return torch.from_numpy(a.view(np.int16).copy()).view(BF16)
    return torch.from_numpy(a.copy())


# (name, value): "zero_v0" also zeroes v there, so Adam's denom is eps alone
SPECIALS = [("zero_v0", 0.0), ("+0", 0.0), ("-0", -0.0), ("denormal+", 1e-40), ("denormal-", -1e-40),
            ("+3e38", 3e38), ("-3e38", -3e38), ("inf", math.inf), ("nan", math.nan)]
SPECIAL_NUMELS = [1, 2, 5, 63, 1023, 1024, 1025, 4095, 4096, 4097, 3, 7, 64, 1, 65, 6]


def _place_specials(numels, g, v):
    """each special value at some tensor's first element and at some tensor's last one"""
    spots = [(t, i) for t, n in enumerate(numels) if n > 1 for i in (0, n - 1)]
    spots += [(t, 0) for t, n in enumerate(numels) if n == 1]
    seen = set()
    for k, (t, i) in enumerate(spots):
        name, val = SPECIALS[k % len(SPECIALS)]
        g[t][i] = val  # the cast to the grad dtype happens in place: a bf16 denormal, a finite bf16 3e38
        if name == "zero_v0" and v is not None:
            v[t][i] = 0.0
        if name.startswith("denormal"):  # still a denormal after the cast, not a zero
            assert 0.0 < abs(float(g[t][i])) < 2.0 ** -126
        if name.endswith("3e38"):  # still finite after the cast
            assert math.isfinite(float(g[t][i])) and abs(float(g[t][i])) > 2.9e38
        seen.add((name, "first" if i == 0 else "last"))
        if numels[t] == 1:
            seen.add((name, "last"))
    assert len(seen) == 2 * len(SPECIALS), "a special value misses an edge"


@functools.lru_cache(maxsize=None)
def _inputs(numels, gdt, seed, special):
    """(p, g, m, v) on the CPU, a few decades of magnitude; v >= 0; m doubles as SGD's buffer"""
    gen = torch.Generator().manual_seed(seed)

    def decade():
        return 10 ** float(torch.randint(-3, 2, (1,), generator=gen))

    p = [torch.randn(n, generator=gen) * decade() for n in numels]
    g = [(torch.randn(n, generator=gen) * decade()).to(gdt) for n in numels]
    m = [torch.randn(n, generator=gen) * decade() for n in numels]
    v = [torch.randn(n, generator=gen).square() * decade() for n in numels]
    if special:
        _place_specials(numels, g, v)
    return p, g, m, v


# -------------------------------------------------------------------- Adam
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=3)


def _adam_scalars():
    bc1 = 1 - ADAM["beta1"] ** ADAM["step"]
    bc2 = 1 - ADAM["beta2"] ** ADAM["step"]
    return (ADAM["lr"] / bc1) * -1, bc2 ** 0.5  # as oracle.adam forms them


@functools.lru_cache(maxsize=None)
def _adam_ref(numels, gdt, ldt, seed, special, maximize, grad_scale, adamw, wd):
    p, g, m, v = _inputs(numels, gdt, seed, special)
    out = [[], [], [], []]
    for t in range(len(numels)):
        r = O.adam(p[t].numpy(), _to_np(g[t]), m[t].numpy(), v[t].numpy(), ADAM["step"], ADAM["lr"], ADAM["beta1"],
                   ADAM["beta2"], ADAM["eps"], wd, adamw, maximize, grad_scale, lowp=LOWP_NAME[ldt])
        for k in range(3):
            out[k].append(torch.from_numpy(r[k]))
        if ldt is not None:
            out[3].append(_from_lowp(r[3], ldt))
    return out


def _check_copy(p_got, lo_got, ldt):
    """the copy is the cast of the STORED fp32 p — torch's cast, or for bf16 the oracle's — and the
    bf16 copy of a NaN is exactly 0x7FC0"""
    for t, (x, lo) in enumerate(zip(p_got, lo_got)):
        if ldt == BF16:
            want = _from_lowp(O.f32_to_bf16(x.numpy()), BF16)
            assert same_bits(lo, want), f"copy: tensor {t} is not f32_to_bf16 of the stored p"
            assert same_bits_nan(lo, x.to(BF16)), f"copy: tensor {t} is not the stored p.to(bf16)"
        else:
            assert same_bits_nan(lo, x.to(ldt)), f"copy: tensor {t} is not the stored p.to({ldt})"


def _adam_launch(device, numels, gdt, ldt, inputs, offs, maximize, grad_scale, found_inf, adamw, wd, hyper, cached):
    p, g, m, v = inputs
    slots = [(F32, p, offs[0]), (gdt, g, offs[1]), (F32, m, offs[2]), (F32, v, offs[3])]
    if ldt is not None:
        slots.append((ldt, None, offs[4]))
    step_size, bc2s = _adam_scalars()

    def launch(plan):
        gs = None if grad_scale is None else _scalar(device, grad_scale)
        fi = None if found_inf is None else _scalar(device, found_inf)
        lr, ss, b2 = ADAM["lr"], step_size, bc2s
        if hyper:  # the source holds the true values; the arguments are deliberately wrong
            src = torch.tensor([step_size, bc2s, 1.0 - ADAM["lr"] * wd, 0.0], dtype=torch.float32, device=device)
            plan.set_hyper_source(src)
            lr, ss, b2 = 123.0, -55.0, 0.5
        if cached:  # a Σg² pass read the grads: the update takes the cached-load instantiation
            plan.sqnorm(1, gdt, torch.zeros(1, dtype=torch.float32, device=device))
        plan.adam(gdt, lr, ADAM["beta1"], ADAM["beta2"], ADAM["eps"], wd, adamw, maximize, ss, b2,
                  lowp_dtype=ldt, grad_scale=gs, found_inf=fi)

    return run_guarded(device, numels, slots, launch)


def run_adam(device, numels, gdt, ldt, maximize=False, grad_scale=None, found_inf=None, hyper=False, cached=False,
             off_slot=None, adamw=True, wd=1e-2, special=False, seed=21):
    """One Adam(W) step on guarded tensors against the oracle: p, exp_avg, exp_avg_sq and the copy
    bit for bit, the grads untouched, the copy the cast of the stored p.  ``found_inf`` = 1: nothing
    changes.  ``hyper`` / ``cached``: the variant launch and the plain one, both against the oracle
    and against each other."""
    numels = tuple(numels)
    inputs = _inputs(numels, gdt, seed, special)
    offs = _slot_offs(5, off_slot)
    args = (device, numels, gdt, ldt, inputs, offs, maximize, grad_scale, found_inf, adamw, wd)
    runs = [_adam_launch(*args, hyper, cached)]
    if hyper or cached:
        runs.append(_adam_launch(*args, False, False))
    if found_inf:
        want = [inputs[0], inputs[2], inputs[3]]
        want_lo = sentinel_list(numels, ldt) if ldt is not None else None
    else:
        ref = _adam_ref(numels, gdt, ldt, seed, special, maximize, grad_scale, adamw, wd)
        want, want_lo = ref[:3], ref[3]
    for got in runs:
        assert_lists(got[0], want[0], "p")
        assert_lists(got[2], want[1], "exp_avg")
        assert_lists(got[3], want[2], "exp_avg_sq")
        assert_lists(got[1], inputs[1], "grads (read-only)", nan_ok=False)
        if ldt is not None:
            assert_lists(got[4], want_lo, "copy", nan_ok=not found_inf)
            if not found_inf:
                _check_copy(got[0], got[4], ldt)
    if len(runs) == 2:
        for s in range(len(runs[0])):
            assert_lists(runs[0][s], runs[1][s], f"variant launch vs plain launch, slot {s}")


# --------------------------------------------------------------------- SGD
SGD = dict(lr=0.1, momentum=0.9, wd=1e-4)


@functools.lru_cache(maxsize=None)
def _sgd_ref(numels, gdt, ldt, seed, special, maximize, grad_scale, momentum, nesterov, first, wd):
    p, g, b, _ = _inputs(numels, gdt, seed, special)
    out = [[], [], []]
    for t in range(len(numels)):
        r = O.sgd(p[t].numpy(), _to_np(g[t]), b[t].numpy(), SGD["lr"], momentum, 0.0, wd, nesterov, maximize,
                  first, grad_scale, lowp=LOWP_NAME[ldt])
        out[0].append(torch.from_numpy(r[0]))
        out[1].append(torch.from_numpy(r[1]))
        if ldt is not None:
            out[2].append(_from_lowp(r[2], ldt))
    return out


def _sgd_launch(device, numels, gdt, ldt, inputs, offs, maximize, grad_scale, found_inf, momentum, nesterov, first,
                wd, hyper, cached):
    p, g, b, _ = inputs
    # the buffer is not read on the first step and not touched without momentum: the sentinel then
    buf = b if (momentum != 0 and not first) else None
    slots = [(F32, p, offs[0]), (gdt, g, offs[1]), (F32, buf, offs[2])]
    if ldt is not None:
        slots.append((ldt, None, offs[3]))

    def launch(plan):
        gs = None if grad_scale is None else _scalar(device, grad_scale)
        fi = None if found_inf is None else _scalar(device, found_inf)
        lr = SGD["lr"]
        if hyper:  # the source holds the true lr; the argument is deliberately wrong
            plan.set_hyper_source(torch.tensor([SGD["lr"], float(first), 0.0], dtype=torch.float32, device=device))
            lr = 123.0
        if cached:  # a Σg² pass read the grads: the update takes the cached-load instantiation
            plan.sqnorm(1, gdt, torch.zeros(1, dtype=torch.float32, device=device))
        plan.sgd(gdt, lr, momentum, 0.0, wd, nesterov, maximize, first, lowp_dtype=ldt, grad_scale=gs, found_inf=fi)

    return run_guarded(device, numels, slots, launch)


def run_sgd(device, numels, gdt, ldt, maximize=False, grad_scale=None, found_inf=None, hyper=False, cached=False,
            off_slot=None, momentum=SGD["momentum"], nesterov=False, first=False, wd=SGD["wd"], special=False,
            seed=22):
    """One SGD step on guarded tensors against the oracle, as :func:`run_adam`.  Without momentum
    slot 2 holds the sentinel and must still hold it afterwards; on the first step it holds the
    sentinel before (the kernel must not read it) and the new buffer after."""
    numels = tuple(numels)
    inputs = _inputs(numels, gdt, seed, special)
    offs = _slot_offs(4, off_slot)
    args = (device, numels, gdt, ldt, inputs, offs, maximize, grad_scale, found_inf, momentum, nesterov, first, wd)
    runs = [_sgd_launch(*args, hyper, cached)]
    if hyper or cached:
        runs.append(_sgd_launch(*args, False, False))
    sentinel = sentinel_list(numels, F32)
    if found_inf:
        want_p, want_b = inputs[0], (inputs[2] if (momentum != 0 and not first) else sentinel)
        want_lo = sentinel_list(numels, ldt) if ldt is not None else None
    else:
        ref = _sgd_ref(numels, gdt, ldt, seed, special, maximize, grad_scale, momentum, nesterov, first, wd)
        want_p, want_b, want_lo = ref[0], (ref[1] if momentum != 0 else sentinel), ref[2]
    exact_buf = bool(found_inf) or momentum == 0  # the sentinel is a NaN: its payload must survive
    for got in runs:
        assert_lists(got[0], want_p, "p")
        assert_lists(got[2], want_b, "momentum buffer", nan_ok=not exact_buf)
        assert_lists(got[1], inputs[1], "grads (read-only)", nan_ok=False)
        if ldt is not None:
            assert_lists(got[3], want_lo, "copy", nan_ok=not found_inf)
            if not found_inf:
                _check_copy(got[0], got[3], ldt)
    if len(runs) == 2:
        for s in range(len(runs[0])):
            assert_lists(runs[0][s], runs[1][s], f"variant launch vs plain launch, slot {s}")


# ------------------------------------------------------------------- scale
SCALES = [("mul", float(np.float32(1.0 / 3.0))), ("div", 3.0), ("div", float(np.float32(0.7))), ("mul", 0.5)]
SCALE_IDS = ["mul-1/3", "div-3", "div-0.7", "mul-0.5"]


@functools.lru_cache(maxsize=None)
def _values(numels, dt, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=gen) * 10 ** float(torch.randint(-3, 3, (1,), generator=gen))).to(dt)
            for n in numels]


def run_scale(device, numels, dt, mode, s, off):
    """gs_scale in place: one IEEE fp32 multiply or divide by fp32(s), one round-to-nearest-even cast"""
    from distributed_training_amd import _lib as L

    numels = tuple(numels)
    x = _values(numels, dt, 31)
    s32 = np.float32(s)
    assert float(s32) == s, "the scale must be an fp32 value: the C ABI takes a float"
    want = []
    for t in x:
        a = t.float().numpy()
        want.append(torch.from_numpy(a / s32 if mode == "div" else a * s32).to(dt))
    (got,) = run_guarded(device, numels, [(dt, x, off)],
                         lambda plan: plan.scale(0, dt, s, L.GS_SCALE_DIV if mode == "div" else L.GS_SCALE_MUL))
    assert_lists(got, want, f"scale {mode} {s}")


# --------------------------------------------------------------------- sum
def run_sum(device, numels, dt, off):
    """gs_sum of integers in [-8, 8]: exact in any order, so the fp64 sum exactly; then accumulated
    once more onto it: twice the sum"""
    numels = tuple(numels)
    total = sum(numels)
    assert 16 * total < 2 ** 24, "partial sums (of two launches) must stay exact in fp32"
    gen = torch.Generator().manual_seed(41)
    x = [torch.randint(-8, 9, (n,), generator=gen).to(dt) for n in numels]
    want = float(sum(t.double().sum() for t in x))
    out = GuardedList([1], F32, device)
    out.fill([torch.tensor([12345.0])])
    seen = []

    def launch(plan):
        plan.sum(0, dt, out.views[0])
        _sync(device)
        seen.append(out.read())
        plan.sum(0, dt, out.views[0], accumulate=True)

    (got,) = run_guarded(device, numels, [(dt, x, off)], launch)
    seen.append(out.read())
    assert_lists(got, x, "sum input (read-only)", nan_ok=False)
    for (val, intact), w in zip(seen, (want, 2 * want)):
        assert intact, "a guard element around the sum's output changed"
        assert float(val[0][0]) == w, (float(val[0][0]), w)


def run_sum_empty(device, numels=()):
    """a plan without elements writes 0 without ``accumulate`` and leaves the output alone with it"""
    out = GuardedList([1], F32, device)
    out.fill([torch.tensor([12345.0])])

    def launch(plan):
        plan.sum(0, F32, out.views[0], accumulate=True)
        _sync(device)
        assert same_bits(out.read()[0][0], torch.tensor([12345.0]))
        plan.sum(0, F32, out.views[0])

    run_guarded(device, tuple(numels), [(F32, [torch.zeros(0)] * len(numels), 0)], launch)
    val, intact = out.read()
    assert intact and same_bits(val[0], torch.tensor([0.0]))


# ----------------------------------------------------------------- unscale
NONFINITE = [math.inf, -math.inf, math.nan]


def unscale_placements(numels):
    """About a dozen (tensor, element, value): the first and the last element of the tensors on both
    sides of the chunk and of the 4 Ki group, of two 1-element tensors, of tensors of a mixed
    chunk of more than 64 tensors, and of the plan's last tensor; +inf, -inf and NaN in turn."""
    numels = list(numels)
    if numels == LIST_A:
        ts = [numels.index(n) for n in (1, 1023, 1024, 1025, 4095, 4096, 4097)] + [len(numels) - 1]
    else:
        assert numels == LIST_B and numels[0] == 1 and numels[63] == 1
        ts = [0, 63, 64, 65, 130, len(numels) - 1]
    spots = []
    for t in ts:
        for i in sorted({0, numels[t] - 1}):
            spots.append((t, i, NONFINITE[len(spots) % 3]))
    return spots


def _unscale_once(device, lists, plan, x, dt, inv, preset):
    """one launch on ``x``; (grads, flag) of the kernel and of torch's CPU kernel"""
    lists.fill(x)
    flag = _scalar(device, preset)
    plan.unscale_check(0, dt, _scalar(device, inv), flag)
    _sync(device)
    got, intact = lists.read()
    assert intact, "a guard element around a grad changed"
    want = [t.clone() for t in x]
    want_flag = torch.tensor([preset])
    torch._amp_foreach_non_finite_check_and_unscale_([t for t in want if t.numel()], want_flag, torch.tensor([inv]))
    return got, float(flag.cpu()[0]), want, float(want_flag[0])


def run_unscale(device, numels, dt, off, nonfinite=False, inv=0.25):
    """gs_unscale_check against torch._amp_foreach_non_finite_check_and_unscale_ on the CPU: the
    clean list (flag 0, and a flag preset to 1 staying 1), or one non-finite value per launch at
    each of :func:`unscale_placements` (flag exactly 1, every other element torch's)"""
    from distributed_training_amd.multi_tensor import TensorListPlan, update_task_units

    numels = tuple(numels)
    x = _values(numels, dt, 51)
    lists = GuardedList(numels, dt, device, off)
    plan = TensorListPlan(numels, device, task_units=update_task_units(device))
    plan.set_ptrs(0, lists.views)
    try:
        if not nonfinite:
            for preset in (0.0, 1.0):  # the flag accumulates: 0 stays 0, 1 stays 1
                got, flag, want, want_flag = _unscale_once(device, lists, plan, x, dt, inv, preset)
                assert flag == preset and want_flag == preset
                assert_lists(got, want, "clean grads", nan_ok=False)
            return
        for t, i, val in unscale_placements(numels):
            bad = [a.clone() if k == t else a for k, a in enumerate(x)]
            bad[t][i] = val
            got, flag, want, want_flag = _unscale_once(device, lists, plan, bad, dt, inv, 0.0)
            assert flag == 1.0 and want_flag == 1.0, (t, i, val, flag)
            assert_lists(got, want, f"{val} at element {i} of tensor {t}")
    finally:
        plan.close()


# NaNs with payloads, quiet and signalling, of both signs, and an infinity: a multiply by 1 or a
# round trip through fp32 and back would rewrite at least the signalling ones
ODD_BITS = {F32: [0x7FC00005, 0x7F800001, -0x3FFFFB, 0x7F800000], BF16: [0x7FC5, 0x7F81, -0x3B, 0x7F80],
            F16: [0x7E05, 0x7C01, -0x1FB, 0x7C00]}


def run_unscale_no_write(device, dt, off, inv):
    """``inv`` None or 1.0: the flag is set, and no grad is written — NaN payloads survive bit for bit"""
    numels = (5, 1025, 4097, 1)
    x = [t.clone() for t in _values(numels, dt, 52)]
    odd = torch.tensor(ODD_BITS[dt], dtype=PATTERN[dt][0])
    bits(x[0])[:4] = odd       # views: the patterns land in x
    bits(x[1])[-4:] = odd
    bits(x[2])[0] = odd[1]
    bits(x[2])[-1] = odd[2]
    bits(x[3])[0] = odd[0]
    for preset in (0.0, 1.0):
        flag = _scalar(device, preset)
        (got,) = run_guarded(device, numels, [(dt, x, off)],
                             lambda plan: plan.unscale_check(0, dt, None if inv is None else _scalar(device, inv), flag))
        assert float(flag.cpu()[0]) == 1.0
        assert_lists(got, x, "grads that must not be written", nan_ok=False)


def run_unscale_f16_overflow(device, off):
    """a finite fp16 grad whose product with inv overflows fp16: inf is stored, the flag stays 0"""
    numels = (5, 1025, 4097, 1)
    x = [t.clone() for t in _values(numels, F16, 53)]
    for t in x:
        t.clamp_(-100, 100)
        t[0] = 60000.0
        t[-1] = -40000.0
    inv = 2.0
    flag = _scalar(device, 0.0)
    (got,) = run_guarded(device, numels, [(F16, x, off)],
                         lambda plan: plan.unscale_check(0, F16, _scalar(device, inv), flag))
    want = [t.clone() for t in x]
    want_flag = torch.zeros(1)
    torch._amp_foreach_non_finite_check_and_unscale_(want, want_flag, torch.tensor([inv]))
    assert float(want_flag[0]) == 0.0 and float(flag.cpu()[0]) == 0.0
    assert all(math.isinf(float(t[0])) and math.isinf(float(t[-1])) for t in got)
    assert_lists(got, want, "overflowing fp16 grads", nan_ok=False)
