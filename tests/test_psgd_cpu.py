"""PowerSGD on the host backend: the four stages exactly on integer operands, the fused hook
over gloo on CPU buckets (world size 2), and the limits the hook names."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests._dist_util import free_port, init_pg
from tests._psgd_ref import check_stages_exact, run_hook_steps


@pytest.mark.parametrize("use_error", [True, False])
@pytest.mark.parametrize("rank", [1, 2, 4, 8])
def test_host_stages_exact(rank, use_error):
    check_stages_exact(torch.device("cpu"), rank, use_error)


def _worker(rank, ws, port, errq):
    try:
        init_pg("gloo", rank, ws, port)
        run_hook_steps(rank, ws, torch.device("cpu"), 2, True, True)
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # report to the parent
        import traceback

        errq.put(f"rank {rank}: {e!r}\n{traceback.format_exc()}")
        raise


def test_hook_ws2_gloo_cpu():
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, errq)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


def test_limits():
    import distributed_training_amd as D

    with pytest.raises(ValueError, match="1..8"):
        D.PowerSGDState(None, matrix_approximation_rank=9, start_powerSGD_iter=2)
    with pytest.raises(ValueError, match="start_powerSGD_iter"):
        D.PowerSGDState(None, start_powerSGD_iter=1, use_error_feedback=True, warm_start=False)
    state = D.PowerSGDState(None, start_powerSGD_iter=2)
    bucket = D.GradBucket(0, torch.zeros(8, dtype=torch.bfloat16), [], [], True)
    with pytest.raises(ValueError, match="fp32 bucket"):
        D.powerSGD_hook(state, bucket)
