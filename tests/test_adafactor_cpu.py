"""FusedAdafactor through the host backend: exact factor sums on integer grads, three steps
against torch.optim.Adafactor in fp64, and the drop-in contract (validation messages, the
tensors it refuses, the state_dict exchange with torch.optim.Adafactor in both directions)."""
from copy import deepcopy

import pytest
import torch

import distributed_training_amd as D
from tests import _adafactor_common as C

STEP_CASES = [(0.0, False, 1.0, 1e-2), (0.1, False, 1.0, 1e-2), (0.0, True, 2.0, 1e-2), (0.01, True, 2.0, 10.0)]


def test_exact_sums():
    C.check_exact_sums("cpu")


@pytest.mark.parametrize("weight_decay,maximize,d,lr", STEP_CASES)
def test_three_steps_against_fp64(weight_decay, maximize, d, lr):
    C.check_three_steps("cpu", weight_decay, maximize, d, lr)


@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(lr=torch.ones(2)), dict(beta2_decay=0.5), dict(eps=(-1.0, 1e-3)),
                                dict(eps=(None, -1.0)), dict(d=0.5), dict(weight_decay=-0.1)])
def test_validation_messages_are_torchs(kw):
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError) as theirs:
        torch.optim.Adafactor(p, **kw)
    with pytest.raises(ValueError) as mine:
        D.FusedAdafactor(p, **kw)
    assert str(mine.value) == str(theirs.value)


@pytest.mark.parametrize("make", [
    lambda: torch.zeros(4, 4, dtype=torch.bfloat16), lambda: torch.zeros(4, 4, dtype=torch.float16),
    lambda: torch.zeros(2, 3, 4), lambda: torch.zeros(2, 2, 2, 2, 2), lambda: torch.zeros(4, 6).t(),
    lambda: torch.zeros(2, 3, 9, 8).contiguous(memory_format=torch.channels_last), lambda: torch.zeros(0)])
def test_unsupported_tensors_raise(make):
    with pytest.raises(ValueError, match="FusedAdafactor"):
        D.FusedAdafactor([torch.nn.Parameter(make())])


def test_state_dict_moves_to_torch_and_back():
    cases = [((7,), False), ((3, 5, 3, 3), True), ((3, 5, 3, 3), False), ((9, 8), False)]
    gen = torch.Generator().manual_seed(19)
    pf = C.copies(C.masters(gen, cases))
    of = D.FusedAdafactor(pf, eps=(None, C.EPS2), weight_decay=0.1)
    C.set_grads(pf, C.grads(gen, cases))
    of.step()
    # into torch: the fp32 and the fp64 optimizer both continue from the fused state (copies: a loaded
    # `step` tensor is the state_dict's own)
    p32, p64 = C.copies(pf), C.copies(pf, dtype=torch.float64)
    o32, o64 = C.torch_opt(p32, weight_decay=0.1), C.torch_opt(p64, weight_decay=0.1)
    o32.load_state_dict(deepcopy(of.state_dict()))
    o64.load_state_dict(deepcopy(of.state_dict()))
    gs = C.grads(gen, cases)
    for ps, opt in ((pf, of), (p32, o32), (p64, o64)):
        C.set_grads(ps, gs)
        opt.step()
    C.assert_within_bound((pf, of), (p32, o32), (p64, o64), cases)
    # and back: a fresh fused optimizer and a fresh fp64 one continue from torch's fp32 state
    pb, q64 = C.copies(p32), C.copies(p32, dtype=torch.float64)
    ob, r64 = D.FusedAdafactor(pb, eps=(None, C.EPS2), weight_decay=0.1), C.torch_opt(q64, weight_decay=0.1)
    ob.load_state_dict(deepcopy(o32.state_dict()))
    r64.load_state_dict(deepcopy(o32.state_dict()))
    gs = C.grads(gen, cases)
    for ps, opt in ((pb, ob), (p32, o32), (q64, r64)):
        C.set_grads(ps, gs)
        opt.step()
    assert all(ob.state[p]["step"].item() == 3 for p in pb)
    C.assert_within_bound((pb, ob), (p32, o32), (q64, r64), cases)
