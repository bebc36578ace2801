"""dist.WideHub(native_head=True): the server rank runs slk_wide_head_mx on the received MX records instead of decode +
head + encode. Three gloo processes on one GPU (two clients of 4 samples in 2 micro-batches, one server), the pattern of
test_cutmx_dist_gpu.py; every rank runs two hub steps with native_head=False and then two, from the same seeded
weights, with native_head=True, and the two runs must agree bit for bit: parameters, logged losses, exchange_bytes."""
import os

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from test_cutmx_dist_gpu import MICRO, WB, WORLD, _port

pytestmark = pytest.mark.gpu

STEPS = 2


def _worker(rank, world, port, outdir, fwd, bwd):
    import sys
    sys.path[:0] = [PKG, ROOT, os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from splitcnn import dist as sd
    from splitcnn.codec import MxCut
    from splitcnn.wide import SyntheticCIFAR, WideClientStage, WideServerStage, init_wide_models
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {}
    try:
        grp = sd.client_group_for(world)
        nc = world - 1
        data = SyntheticCIFAR(17)
        batches = [tuple(t.to(dev) for t in data.batch(nc * WB)) for _ in range(STEPS)]
        for native in (False, True):
            wa, wb = init_wide_models(seed=0)
            stage = WideClientStage(wa, device=dev) if rank < nc else WideServerStage(wb, device=dev)
            t = sd.WideHub(stage, rank, world, client_group=grp, micro=MICRO, codec=MxCut(fwd=fwd, bwd=bwd),
                           native_head=native)
            for x, y in batches:
                if rank < nc:
                    sl = slice(rank * WB, (rank + 1) * WB)
                    t.client_step(x[sl].contiguous(), y[sl].contiguous())
                else:
                    t.server_step(WB, dev, WideClientStage.cut_shape, WideClientStage.cut_dtype)
            torch.cuda.synchronize()
            t.check_exchange()
            tag = "native" if native else "plain"
            if rank == nc:
                res["losses_" + tag] = np.array([l for _, l in stage.loss_log.flush()])
                res["dense_buffers_" + tag] = np.array([k[0] in ("cuts", "dcuts") for k in t._bufs]).sum()
            res["params_" + tag] = stage.params.cpu().numpy()
            res["bytes_" + tag] = np.array([t.exchange_bytes, t.dense_bytes])
        np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("fwd,bwd", [("e2m1", "e2m1"), ("e4m3", None)])
def test_native_head_step_is_bitwise_the_plain_step(gpu, tmp_path, fwd, bwd):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(WORLD, _port(), str(tmp_path), fwd, bwd), nprocs=WORLD, join=True)
    out = [dict(np.load(os.path.join(tmp_path, f"r{r}.npz"))) for r in range(WORLD)]
    for r in range(WORLD):
        assert np.array_equal(out[r]["params_native"].view(np.int32), out[r]["params_plain"].view(np.int32)), f"rank {r}"
        assert np.array_equal(out[r]["bytes_native"], out[r]["bytes_plain"])
    srv = out[WORLD - 1]
    assert len(srv["losses_plain"]) == STEPS and np.isfinite(srv["losses_plain"]).all()
    assert np.array_equal(srv["losses_native"].view(np.int32), srv["losses_plain"].view(np.int32))
    # the native server keeps no dense cut, and a dense gradient buffer only where that direction is dense
    assert int(srv["dense_buffers_plain"]) == 2 and int(srv["dense_buffers_native"]) == (0 if bwd else 1)


def test_native_head_refusals(gpu):
    from splitcnn import dist as sd
    from splitcnn.codec import Fp8Cut, MxCut
    from splitcnn.loss import SoftCrossEntropy
    from splitcnn.wide import WideServerStage
    stage = WideServerStage(device=gpu)
    for codec in (Fp8Cut(), None, MxCut(fwd=None, bwd="e2m1")):
        with pytest.raises(ValueError, match="native_head"):
            sd.WideHub(stage, 2, 3, codec=codec, native_head=True)
    soft = WideServerStage(device=gpu, loss=SoftCrossEntropy(0.1))
    with pytest.raises(ValueError, match="soft-target"):
        sd.WideHub(soft, 2, 3, codec=MxCut(), native_head=True)
    with pytest.raises(ValueError, match="soft-target"):
        soft.forward_backward_records(None, "e2m1", None, 1.0, None, None)
    sd.WideHub(stage, 0, 3, codec=MxCut(), native_head=True)   # a client rank accepts the flag
