"""The bf16-state route of the row-sharded UVd driver (psgd_tf_amd/sharded.py) under gloo on CPU.

A NumPy stage backend (tests/cpu_stages_bf16.py: fp64 arithmetic, round to nearest even) stands in for the HIP stages, so what
is under test is the choreography: how many exchanges a call makes and of which stages, in the same order on both ranks (apply
2, update 2, fused step 4, one more on the balance branch), the one set-up collective behind row0, and that the 2-rank result
equals the 1-rank result of the same backend."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.uvd_cases import make_uvd_problem, rel_err

N, R = 1003, 6
TINY = float(np.finfo(np.float32).tiny)
KEYS = ("U", "V", "d", "o_apply", "o_f1", "o_f0")


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from psgd_tf_amd import sharded
        from tests.cpu_stages_bf16 import NumpyBf16Stages
        calls = {"all_gather_into_tensor": 0, "all_reduce": 0, "broadcast": 0}
        for name in calls:
            def wrap(fn, name=name):
                def counted(*a, **k):
                    calls[name] += 1
                    return fn(*a, **k)
                return counted
            setattr(dist, name, wrap(getattr(dist, name)))
        p = make_uvd_problem(N, R, seed=21, uv_gain=2.0, d_spread=0.3)
        p["U"] *= 5.0
        lo, hi = sharded.shard_rows(N, rank, world)
        t = {k: torch.from_numpy(p[k][lo:hi].copy()) for k in p}
        for k in ("U", "V", "d"):
            t[k] = t[k].to(torch.bfloat16)
        be = NumpyBf16Stages(R)
        record = []          # (call, collectives, stages exchanged)

        def run(name, fn):
            c0, l0 = dict(calls), len(be.log)
            out = fn()
            record.append((name, {k: calls[k] - c0[k] for k in calls}, list(be.log[l0:])))
            return out
        kw = dict(backend=be, rounding="nearest")
        # the first updating call looks up row0: ONE set-up collective, never again for this (group, row count)
        run("update+setup", lambda: sharded.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], 0.01, TINY, balance=False,
                                                                     update_U=True, **kw))
        assert be.narrow_args[-1][3] == lo and be.narrow_args[-2][3] == lo           # row0 = rows on the ranks before this one
        run("update", lambda: sharded.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], 0.01, TINY, balance=False,
                                                               update_U=False, **kw))
        run("update_balance", lambda: sharded.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], 0.01, TINY,
                                                                       balance=True, update_U=True, **kw))
        o_apply = run("apply", lambda: sharded.precond_grad_UVd_math(t["U"], t["V"], t["d"], t["g"], backend=be))
        o_f1 = run("fused", lambda: sharded.update_precond_UVd_math_and_precond_grad(
            t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], 0.01, TINY, balance=False, update_U=True, **kw))
        o_f0 = run("fused_balance", lambda: sharded.update_precond_UVd_math_and_precond_grad(
            t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], 0.01, TINY, balance=True, update_U=False, **kw))
        # an explicit row0 is passed through; one seed for every narrowing stage of a call
        run("update_row0", lambda: sharded.update_precond_UVd_math_(t["U"].clone(), t["V"].clone(), t["d"].clone(), t["v"], t["h"], 0.01,
                                                                    TINY, balance=False, update_U=True, backend=be,
                                                                    rounding="stochastic", rounding_seed=77, row0=12345))
        assert be.narrow_args[-2:] == [("rewrite", 1, 77, 12345), ("d", 1, 77, 12345)]
        want = {"update+setup": (3, [11, 12]), "update": (2, [11, 12]), "update_balance": (3, [10, 11, 12]), "apply": (2, [1, 2]),
                "fused": (4, [11, 12, 1, 2]), "fused_balance": (5, [10, 11, 12, 1, 2]), "update_row0": (2, [11, 12])}
        for name, c, stages in record:
            assert c == {"all_gather_into_tensor": want[name][0], "all_reduce": 0, "broadcast": 0}, (name, c)
            assert stages == want[name][1], (name, stages)
        assert all(t[k].dtype == torch.bfloat16 for k in ("U", "V", "d"))
        # a mixed state, a rank above 32 and rounding arguments on an fp32 state are refused before anything is exchanged
        with pytest.raises(TypeError, match="mixed"):
            sharded.precond_grad_UVd_math(t["U"], t["V"].float(), t["d"], t["g"], backend=be)
        with pytest.raises(ValueError, match="32"):
            sharded.precond_grad_UVd_math(torch.zeros(8, 40, dtype=torch.bfloat16), torch.zeros(8, 40, dtype=torch.bfloat16),
                                          torch.ones(8, 1, dtype=torch.bfloat16), torch.ones(8, 1), backend=be)
        with pytest.raises(ValueError, match="bfloat16 state only"):
            sharded.update_precond_UVd_math_(t["U"].float(), t["V"].float(), t["d"].float(), t["v"], t["h"], 0.01, TINY, balance=False,
                                             update_U=True, backend=be, row0=3)
        with pytest.raises(ValueError, match="rounding"):
            sharded.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], 0.01, TINY, balance=False, update_U=True,
                                             backend=be, rounding="up")
        np.savez(os.path.join(outdir, "w%d_rank%d.npz" % (world, rank)), U=t["U"].float().numpy(), V=t["V"].float().numpy(),
                 d=t["d"].float().numpy(), o_apply=o_apply.numpy(), o_f1=o_f1.numpy(), o_f0=o_f0.numpy(),
                 order=np.array([s for _, _, st in record for s in st]))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_bf16_route_exchanges_and_two_ranks_equal_one():
    with tempfile.TemporaryDirectory() as outdir:
        mp.spawn(_worker, args=(2, _free_port(), outdir), nprocs=2, join=True)
        mp.spawn(_worker, args=(1, _free_port(), outdir), nprocs=1, join=True)
        two = [np.load(os.path.join(outdir, "w2_rank%d.npz" % k)) for k in range(2)]
        one = np.load(os.path.join(outdir, "w1_rank0.npz"))
    assert np.array_equal(two[0]["order"], two[1]["order"])                   # the same exchanges in the same order on both ranks
    assert np.array_equal(two[0]["order"], one["order"])
    for k in ("U", "V", "d"):                                                 # the stored bf16 values do not depend on the split
        assert np.array_equal(np.concatenate([q[k] for q in two], 0), one[k]), k
    for k in ("o_apply", "o_f1", "o_f0"):                                     # fp64 sums folded in another order
        assert rel_err(np.concatenate([q[k] for q in two], 0), one[k]) < 1e-12, k
    assert np.all(np.isfinite(one["o_f0"])) and np.linalg.norm(one["o_f0"]) > 0
