"""dist.WideHub(noise=privacy.CutNoise(...)): three gloo processes on one GPU — two client ranks of 4 samples in 2
micro-batches feed one server rank — against the fused wide.WideTrainer(cut_noise=...) step at the concatenated batch
of 8, with and without the FP8 codec: every part is clipped and noised under the client's step counter and its first
row in the concatenated batch, so the draws are the fused step's. Modelled on tests/test_cut8_sr_dist_gpu.py, to its
tolerances: loss 1e-6 relative, client and server gradients 1e-6 of their maximum."""
import os
import socket

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

WB, MICRO, WORLD, SEED = 4, 2, 3, 5
SCALE, CLIP = 0.3, 31.9   # the norms of the cut at initialisation lie between 30.4 and 32.3: the bound binds on some rows only


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _codec(on):
    from splitcnn.codec import Fp8Cut
    return Fp8Cut("e4m3", "e5m2") if on else None


def _noise():
    from splitcnn.privacy import CutNoise
    return CutNoise("laplace", scale=SCALE, clip=CLIP, seed=SEED)


def _worker(rank, world, port, outdir, with_codec):
    import sys
    sys.path[:0] = [PKG, ROOT, os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from splitcnn import dist as sd
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
        if rank < nc:
            t = sd.WideHub(WideClientStage(wa, device=dev), rank, world, client_group=grp, micro=MICRO,
                           codec=_codec(with_codec), noise=_noise())
            sl = slice(rank * WB, (rank + 1) * WB)
            t.client_step(x[sl].contiguous(), y[sl].contiguous())
            res["stats"] = torch.cat([t._buf(("cut_stats", k), (WB // MICRO, 2), torch.float32, dev)
                                      for k in range(MICRO)]).cpu().numpy()
        else:
            t = sd.WideHub(WideServerStage(wb, device=dev), rank, world, client_group=grp, micro=MICRO,
                           codec=_codec(with_codec))
            t.server_step(WB, dev, WideClientStage.cut_shape, WideClientStage.cut_dtype)
            torch.cuda.synchronize()
            res["losses"] = np.array([l for _, l in t.stage.loss_log.flush()])
        torch.cuda.synchronize()
        t.check_exchange()
        res["step_ctr"] = t.stage.step_ctr.cpu().numpy()
        res["params"] = t.stage.params.cpu().numpy()
        res["grads"] = t.stage.grads.cpu().numpy()
        res["bytes"] = np.array([t.exchange_bytes, t.dense_bytes])
        np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("with_codec", [False, True], ids=["dense", "fp8"])
def test_widehub_noised_exchange_vs_fused_step(gpu, tmp_path, with_codec):
    import torch.multiprocessing as mp
    from splitcnn.wide import SyntheticCIFAR, WideTrainer, init_wide_models
    mp.spawn(_worker, args=(WORLD, _port(), str(tmp_path), with_codec), nprocs=WORLD, join=True)
    out = [dict(np.load(os.path.join(tmp_path, f"r{r}.npz"))) for r in range(WORLD)]
    x, y = SyntheticCIFAR(17).batch(2 * WB)
    ref = WideTrainer(*init_wide_models(seed=0), device=gpu, graph=False, cut_codec=_codec(with_codec),
                      cut_noise=_noise())
    ref.step(x.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    (_, ref_loss), = ref.loss_log.flush()
    assert abs(float(out[2]["losses"][0]) - ref_loss) <= 1e-6 * abs(ref_loss)

    def close(g, w):
        assert np.abs(g - w).max() <= 1e-6 * np.abs(w).max()
    close(out[0]["grads"].astype(np.float64), ref.client.grads.double().cpu().numpy())
    close(out[2]["grads"].astype(np.float64), ref.server.grads.double().cpu().numpy())
    # the clip's pairs are the fused step's rows, bit for bit: the norm is per sample
    stats = ref.cut_stats().numpy()
    assert np.array_equal(np.concatenate([out[0]["stats"], out[1]["stats"]]), stats)
    assert (stats[:, 1] < 1).any() and (stats[:, 1] == 1).any()
    # both clients are bit-identical
    assert np.array_equal(out[0]["params"], out[1]["params"]) and np.array_equal(out[0]["grads"], out[1]["grads"])
    # the byte counts do not change
    per = 2 * 16400 if with_codec else 2 * 32768
    for r, n in ((0, WB), (1, WB), (2, 2 * WB)):
        moved, dense = (int(v) for v in out[r]["bytes"])
        assert moved == n * (per + 8) and dense == n * (2 * 32768 + 8)
    for r in range(WORLD):
        assert int(out[r]["step_ctr"][0]) == 1
    # the defence is what moved: the plain fused step ends elsewhere, beyond the tolerance
    plain = WideTrainer(*init_wide_models(seed=0), device=gpu, graph=False, cut_codec=_codec(with_codec))
    plain.step(x.to(gpu), y.to(gpu))
    g, w = plain.client.grads.double().cpu().numpy(), ref.client.grads.double().cpu().numpy()
    assert np.abs(g - w).max() > 1e-6 * np.abs(w).max()


def test_refusals(gpu):
    from splitcnn import dist as sd
    from splitcnn.privacy import CutNoise

    class Stage:
        def __init__(self, device):
            self.device = device

    with pytest.raises(TypeError, match="CutNoise"):
        sd.WideHub(Stage("cpu"), 0, 3, groups=(None, None), noise=0.5)
    with pytest.raises(ValueError, match="CPU stages"):
        sd.WideHub(Stage("cpu"), 0, 3, groups=(None, None), noise=CutNoise(scale=0.1))
    with pytest.raises(ValueError, match="client ranks"):
        sd.WideHub(Stage(gpu), 2, 3, groups=(None, None), noise=CutNoise(scale=0.1))
