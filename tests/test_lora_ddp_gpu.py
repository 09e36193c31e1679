"""PiZeroDDP with a LoRA model: 2 ranks on one GPU (gloo), in the style of tests/test_ddp_gpu.py.

Rank r trains on samples {2r, 2r+1} of a 4-sample tiny batch as 2 micro-batches (the first under no_sync).  The
averaged adapter gradients must equal one process's on the whole batch within that test's bound, the adapter region
must be reduced exactly once per step, and the frozen base VLM region must not be reduced at all.
"""

import os

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_ddp_gpu import _free_port

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q):
    try:
        import sys

        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path.insert(0, root)
        sys.path.insert(0, os.path.join(root, "open-pi-zero_amd"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch.distributed as dist

        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from oracle.pizero_oracle import TINY_DIMS
        from pizero_native.ddp import PiZeroDDP
        from tests.pizero_gpu_helpers import gpu_inputs
        from tests.test_lora_gpu import build_lora_model

        d = TINY_DIMS
        m = build_lora_model(d)
        gi = gpu_inputs(m, d, 4)
        res = {}

        def mb(idx):
            sl = slice(idx, idx + 1)
            return dict(input_ids=gi["input_ids"][sl], pixel_values=gi["pixel_values"][sl],
                        causal_mask=gi["causal_mask"][sl], vlm_position_ids=gi["vpos"][sl],
                        proprio_position_ids=gi["ppos"][sl], action_position_ids=gi["apos"][sl],
                        proprios=gi["proprios"][sl], actions=gi["actions32"][sl], t=gi["t32"][sl],
                        noise=gi["x0"][sl])

        w = PiZeroDDP(m, bucket_bytes=1 << 16)
        regions = []
        orig_launch = w.reducer._launch

        def launch(region, lo, hi, streams=()):
            regions.append((region, lo, hi))
            return orig_launch(region, lo, hi, streams)

        w.reducer._launch = launch
        m.zero_grad(set_to_none=True)
        with w.no_sync():
            (w(**mb(2 * rank)) / 2).backward()
        (w(**mb(2 * rank + 1)) / 2).backward()
        torch.cuda.synchronize()
        ar = m._arena
        lo, hi = ar.region_range["lora"]
        res["lora_launches"] = [(a, b) for r, a, b in regions if r == "lora"]
        res["lora_covered_once"] = res["lora_launches"] == [(lo, (hi + 7) // 8 * 8)]
        res["vlm_launches"] = sum(1 for r, _, _ in regions if r == "vlm")
        res["action_launches"] = sum(1 for r, _, _ in regions if r == "action")
        gavg = ar.grad.float().clone()
        gl = [torch.empty_like(gavg) for _ in range(world)]
        dist.all_gather(gl, gavg)
        res["ranks_equal"] = torch.equal(gl[0], gl[1])
        if rank == 0:
            eng = m._engine()
            eng.hook = eng.post_backward = None
            m._ddp_wrapper = None
            dist.destroy_process_group()
            m.zero_grad(set_to_none=True)
            loss = m(input_ids=gi["input_ids"], pixel_values=gi["pixel_values"], causal_mask=gi["causal_mask"],
                     vlm_position_ids=gi["vpos"], proprio_position_ids=gi["ppos"], action_position_ids=gi["apos"],
                     proprios=gi["proprios"], actions=gi["actions32"], t=gi["t32"], noise=gi["x0"])
            loss.backward()
            torch.cuda.synchronize()
            gref = ar.grad.float()
            worst, n_lora = 0.0, 0
            for n in ar.order:
                if not m._requires_grad(n):
                    continue
                a, b = ar.view(n, gavg), ar.view(n, gref)
                nb = float(b.norm())
                if nb > 0:
                    worst = max(worst, float((a - b).norm()) / nb)
                    n_lora += "lora_" in n
            res["worst_rel"], res["n_lora"] = worst, n_lora
        else:
            dist.destroy_process_group()
        q.put((rank, res))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, {"error": repr(e), "tb": traceback.format_exc()}))


@pytest.mark.timeout(600)
def test_lora_ddp_two_ranks_one_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = dict(q.get(timeout=540) for _ in ps)
    for p in ps:
        p.join(timeout=60)
    for r in (0, 1):
        assert "error" not in res[r], res[r]
        assert res[r]["lora_covered_once"], res[r]
        assert res[r]["vlm_launches"] == 0 and res[r]["action_launches"] >= 1, res[r]
        assert res[r]["ranks_equal"], res[r]
    print("LoRA DDP vs single-process worst per-tensor rel-L2:", res[0]["worst_rel"], "over", res[0]["n_lora"], "adapters")
    assert res[0]["n_lora"] >= 50
    assert res[0]["worst_rel"] < 2e-2, res[0]
