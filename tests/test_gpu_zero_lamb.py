"""LAMB and LARS under ZeRO-1/2 and 16-bit on the GPU: the HIP update kernels' low-precision
copy (gs_lars_step_lowp / gs_lamb_step_lowp; LarsOp / LambOp with the LD store), and the
sharded step of ZeroDataParallel(optimizer="lamb" | "lars") against the numpy float32
restatements (tests/_zero_lamb_common.py): world 1 over RCCL on the library communicator,
world 2 as two ranks sharing GPU 0 over gloo."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _zero_lamb_common as Z
from tests._dist_util import free_port, init_pg

pytestmark = pytest.mark.gpu


# ---- 1. the update kernels with the copy
# "aligned": the 20480- and 70001-element tensors take the full-chunk path with the copy
# store (st<LD, 4, true> of LambOp / LarsOp); "offset": every tensor takes the checked path
@pytest.mark.parametrize("placement", Z.PLACEMENTS)
@pytest.mark.parametrize("ldt", [torch.bfloat16, torch.float16])
def test_lamb_step_lowp(cuda_device, ldt, placement):
    Z.run_lamb_lowp(cuda_device, ldt, placement)


@pytest.mark.parametrize("placement", Z.PLACEMENTS)
@pytest.mark.parametrize("mom", [0.9, 0.0])
@pytest.mark.parametrize("ldt", [torch.bfloat16, torch.float16])
def test_lars_step_lowp(cuda_device, ldt, mom, placement):
    Z.run_lars_lowp(cuda_device, ldt, mom, placement)


@pytest.mark.parametrize("ldt", [torch.bfloat16, torch.float16])
def test_pieces_off_a_4_element_boundary(cuda_device, ldt):
    Z.run_unaligned_pieces(cuda_device, ldt)


# ---- 2. / 3. / 5. the sharded step, world 1 over RCCL
@pytest.fixture(scope="module")
def rccl_pg(cuda_device):
    if dist.is_initialized():
        yield
        return
    init_pg("nccl", 0, 1, free_port())
    yield
    from distributed_training_amd.comm import destroy_communicators

    destroy_communicators()
    dist.destroy_process_group()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("stage", [1, 2])
def test_sharded_lamb_step_ws1_rccl(cuda_device, rccl_pg, stage, dtype):
    Z.sharded_step_vs_restatement(0, 1, cuda_device, "lamb", stage, dtype)


def test_sharded_lamb_step_applies_the_trust_clamp_ws1_rccl(cuda_device, rccl_pg):
    Z.sharded_step_vs_restatement(0, 1, cuda_device, "lamb", 2, torch.bfloat16, clamp=Z.CLAMP)


def test_sharded_lars_step_ws1_rccl(cuda_device, rccl_pg):
    Z.sharded_step_vs_restatement(0, 1, cuda_device, "lars", 2, torch.bfloat16)


def test_sharded_lamb_full_chunk_path_resnet18_ws1_rccl(cuda_device, rccl_pg):
    """ResNet-18's tensors own full chunk groups (the F = true path with the copy store) inside
    ZeRO's own layout; the plan-level "aligned" cases above cover it per dtype and momentum."""
    Z.sharded_step_vs_restatement(0, 1, cuda_device, "lamb", 2, torch.bfloat16, model="resnet18", steps=1,
                                  bucket=int(4e6))


# ---- world 2 on one GPU
def _gpu_ws2_worker(rank, ws, port, errq, kind, stage, dtype):
    try:
        init_pg("gloo", rank, ws, port)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        Z.sharded_step_vs_restatement(rank, ws, dev, kind, stage, dtype)
        import gc

        gc.collect()  # as tests/test_ddp_cpu.py::_wrap: no gloo work outlives the interpreter
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        import traceback

        errq.put(f"rank {rank}: {e!r}\n{traceback.format_exc()}")
        raise


def _run_ws2(kind, stage, dtype):
    ctx = mp.get_context("spawn")
    errq = ctx.SimpleQueue()
    port = free_port()
    procs = [ctx.Process(target=_gpu_ws2_worker, args=(r, 2, port, errq, kind, stage, dtype)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not errs, "\n".join(errs)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("stage", [1, 2])
def test_sharded_lamb_step_ws2_one_gpu(cuda_device, stage, dtype):
    _run_ws2("lamb", stage, dtype)


def test_sharded_lars_step_ws2_one_gpu(cuda_device):
    _run_ws2("lars", 2, torch.bfloat16)
