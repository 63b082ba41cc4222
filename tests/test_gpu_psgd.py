"""PowerSGD's grouped kernels (gs_psgd_*) and the fused comm hook on the GPU.

Stages: exact on integer operands; the orthogonalisation against fp64 modified
Gram-Schmidt, bounded by 2x the error of torch's own _orthogonalize_gram_schmidt in fp32 on
the same inputs (the margin covers another summation order); same input, same bits.
Hook: micro_resnet at world size 1 over RCCL and 2 over gloo against the fp64 restatement."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch.distributed.algorithms.ddp_comm_hooks.powerSGD_hook import _orthogonalize_gram_schmidt

from tests._dist_util import free_port, init_pg
from tests._psgd_ref import SHAPES, bind, check_stages_exact, mgs, rel_err, run_hook_steps, stage_plan

pytestmark = pytest.mark.gpu
RANKS = [1, 2, 4, 8]


@pytest.mark.parametrize("use_error", [True, False])
@pytest.mark.parametrize("rank", RANKS)
def test_stages_exact(cuda_device, rank, use_error):
    check_stages_exact(cuda_device, rank, use_error)


@pytest.mark.parametrize("eps", [0.0, 1e-8])
@pytest.mark.parametrize("rank", RANKS)
def test_orthogonalize(cuda_device, rank, eps):
    plan, lay, _, _ = stage_plan(cuda_device, rank)
    worst = {}  # (which, tensor) -> [ours, torch's] for the error and for max|XᵀX - I|
    for seed in range(3):
        gen = torch.Generator().manual_seed(seed)
        mem = [torch.randn(lay[k], generator=gen).to(cuda_device) for k in ("p_total", "q_total")]
        x0 = [x.clone() for x in mem]
        for which in (0, 1):
            plan.psgd_orthogonalize(which, mem[which], eps)
            for ti, t in enumerate(lay["tensors"]):
                rows, r, o = t["m" if which else "n"], t["r"], t["q" if which else "p"]
                x = x0[which][o:o + rows * r].view(rows, r)
                ref = mgs(x.double().cpu(), eps)
                theirs = x.clone().unsqueeze(0)
                _orthogonalize_gram_schmidt(theirs, eps)
                w = worst.setdefault((which, ti), [0.0, 0.0, 0.0, 0.0])
                eye = torch.eye(r, dtype=torch.float64)
                for k, y in ((0, mem[which][o:o + rows * r].view(rows, r)), (1, theirs[0])):
                    y = y.double().cpu()
                    w[k] = max(w[k], rel_err(y, ref))
                    w[2 + k] = max(w[2 + k], (y.t() @ y - eye).abs().max().item())
    for (which, ti), (e, et, o, ot) in worst.items():
        print(f"psgd orth rank {rank} eps {eps} {'Q' if which else 'P'} of {SHAPES[ti]}: err {e:.3e} (torch {et:.3e}, "
              f"ratio {e / et:.2f}) orthogonality {o:.3e} (torch {ot:.3e})")
        assert e <= 2 * et and o <= 2 * ot, (which, SHAPES[ti], e, et, o, ot)
    if eps:  # an all-zero column comes out zero, not NaN
        p, t = x0[0].clone(), lay["tensors"][-1]
        col0 = p[t["p"]:].view(t["n"], t["r"])[:, 0]
        col0.zero_()
        plan.psgd_orthogonalize(0, p, eps)
        assert torch.isfinite(p).all() and (col0 == 0).all()


@pytest.mark.parametrize("rank", [1, 8])
def test_same_input_same_bits(cuda_device, rank):
    plan, lay, offs, total = stage_plan(cuda_device, rank)
    gen = torch.Generator().manual_seed(7)
    init = [torch.randn(k, generator=gen).to(cuda_device) for k in (total, total, lay["p_total"], lay["q_total"])]
    runs = []
    for _ in range(2):
        b, e, p, q = (x.clone() for x in init)
        bind(plan, offs, b, e)
        plan.psgd_orthogonalize(1, q)
        plan.psgd_project(True, p, q)
        plan.psgd_orthogonalize(0, p)
        plan.psgd_backproject(p, q)
        plan.psgd_reconstruct(p, q, 0.5)
        runs.append((b, e, p, q))
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    assert all(torch.isfinite(x).all() for x in runs[0])


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("cfg", [(1, True, True), (4, True, True), (2, False, False)])
def test_hook_ws1_rccl(cuda_device, cfg, channels_last):
    owned = False
    if not dist.is_initialized():
        init_pg("nccl", 0, 1, free_port())
        owned = True
    try:
        if dist.get_backend() != "nccl":
            pytest.skip("another module left a non-RCCL default group")
        state, ref = run_hook_steps(0, 1, cuda_device, *cfg, channels_last=channels_last)
        if not channels_last and cfg[2]:  # torch's lengths: Σ n·r and Σ m·r over the compressed tensors
            assert {b: (state.p_memory_dict[b].numel(), state.q_memory_dict[b].numel()) for b in ref.lengths} == \
                ref.lengths
    finally:
        if owned:
            from distributed_training_amd.comm import destroy_communicators

            destroy_communicators()
            dist.destroy_process_group()


def _ws2_worker(rank, ws, port, errq):
    try:
        init_pg("gloo", rank, ws, port)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        run_hook_steps(rank, ws, dev, 2, True, True)
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # report to the parent
        import traceback

        errq.put(f"rank {rank}: {e!r}\n{traceback.format_exc()}")
        raise


def test_hook_ws2_one_gpu_gloo(cuda_device):
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    port = free_port()
    procs = [ctx.Process(target=_ws2_worker, args=(r, 2, port, errq)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
