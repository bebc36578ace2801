"""dist.WideHub(codec=codec.MxCut(...)): three gloo processes on one GPU — two client ranks of 4 samples in 2
micro-batches feed one server rank — against the fused wide.WideTrainer(cut_codec=...) step at the concatenated batch
of 8. The tolerances are those of test_cut8_dist_gpu.py (the summation order differs in the same way): loss 1e-6
relative, client and server gradients 1e-6 of their maximum. They rest on each part's cut and cut gradient entering the
quantiser with the fused step's bits: every rank dumps what it quantised and what came out, and the test first holds
those to the fused step's buffers bit for bit, so a miss of the tolerance can be told from differing quantiser inputs."""
import os
import socket

import numpy as np
import pytest
import torch

import cutmx_ref as Rmx
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

WB, MICRO, WORLD = 4, 2, 3


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


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
        x, y = SyntheticCIFAR(17).batch(nc * WB)
        x, y = x.to(dev), y.to(dev)
        wa, wb = init_wide_models(seed=0)
        codec = MxCut(fwd=fwd, bwd=bwd)
        if rank < nc:
            t = sd.WideHub(WideClientStage(wa, device=dev), rank, world, client_group=grp, micro=MICRO, codec=codec)
            sl = slice(rank * WB, (rank + 1) * WB)
            t.client_step(x[sl].contiguous(), y[sl].contiguous())
        else:
            t = sd.WideHub(WideServerStage(wb, device=dev), rank, world, client_group=grp, micro=MICRO, codec=codec)
            t.server_step(WB, dev, WideClientStage.cut_shape, WideClientStage.cut_dtype)
            torch.cuda.synchronize()
            res["losses"] = np.array([l for _, l in t.stage.loss_log.flush()])
        torch.cuda.synchronize()
        t.check_exchange()
        res["flag"] = t.err_flag.cpu().numpy()
        res["params"] = t.stage.params.cpu().numpy()
        res["grads"] = t.stage.grads.cpu().numpy()
        res["bytes"] = np.array([t.exchange_bytes, t.dense_bytes])
        # what came out of the quantisers on this rank, as int16 bits: the decoded cuts the head read and its dcuts
        # (server), the decoded cut gradient the client back-propagated
        if rank < nc:
            res["dcut"] = t._buf("dcut", WideClientStage.cut_shape(WB), torch.bfloat16, dev).view(torch.int16).cpu().numpy()
        else:
            for name in ("cuts", "dcuts"):
                res[name] = t._buf(name, WideClientStage.cut_shape(nc * WB), torch.bfloat16, dev).view(torch.int16).cpu().numpy()
        np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("fwd,bwd", [("e2m1", "e4m3"), ("e2m1", None)])
def test_widehub_mx_exchange_vs_fused_step(gpu, tmp_path, fwd, bwd):
    import torch.multiprocessing as mp
    from splitcnn.codec import MxCut
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    mp.spawn(_worker, args=(WORLD, _port(), str(tmp_path), fwd, bwd), nprocs=WORLD, join=True)
    out = [dict(np.load(os.path.join(tmp_path, f"r{r}.npz"))) for r in range(WORLD)]
    x, y = SyntheticCIFAR(17).batch(2 * WB)
    ref = WideTrainer(*init_wide_models(seed=0), device=gpu, graph=False, cut_codec=MxCut(fwd=fwd, bwd=bwd))
    ref.step(x.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    (_, ref_loss), = ref.loss_log.flush()
    # the quantisers' outputs against the fused step's buffers, bit for bit (printed: shown if anything below fails):
    # equal bits here mean every part entered the quantiser with the fused step's bits
    shape = (2 * WB, 32, 8, 8, 8)
    head_in = ref.server._b("cut_q", shape, torch.bfloat16).view(torch.int16).cpu().numpy()
    client_in = ref.server._b("dcut", shape, torch.bfloat16).view(torch.int16).cpu().numpy()
    hub_dcut = np.concatenate([out[0]["dcut"], out[1]["dcut"]])
    print("decoded cuts differing from the fused step's:", int((out[2]["cuts"] != head_in).sum()),
          "; back-propagated cut gradients differing:", int((hub_dcut != client_in).sum()),
          "; loss", float(out[2]["losses"][0]), "against", ref_loss)
    assert abs(float(out[2]["losses"][0]) - ref_loss) <= 1e-6 * abs(ref_loss)

    def close(g, w):
        assert np.abs(g - w).max() <= 1e-6 * np.abs(w).max()
    close(out[0]["grads"].astype(np.float64), ref.client.grads.double().cpu().numpy())
    close(out[2]["grads"].astype(np.float64), ref.server.grads.double().cpu().numpy())
    # both clients are bit-identical
    assert np.array_equal(out[0]["params"], out[1]["params"]) and np.array_equal(out[0]["grads"], out[1]["grads"])
    # bytes, exactly: records in every MX direction, dense bf16 otherwise, plus the int64 labels
    fwd_bytes = Rmx.RECORD[fwd]
    back = Rmx.RECORD[bwd] if bwd is not None else 32768
    assert fwd_bytes == 8720 and back in (16912, 32768)
    for r, n in ((0, WB), (1, WB), (2, 2 * WB)):
        moved, dense = (int(v) for v in out[r]["bytes"])
        assert moved == n * (fwd_bytes + back + 8) and dense == n * (2 * 32768 + 8) and moved < dense
    # no malformed record anywhere (the clients decode only when the gradient travels as records)
    for r in range(WORLD):
        assert not out[r]["flag"].any()
