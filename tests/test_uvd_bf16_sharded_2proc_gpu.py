"""GPU, separate PROCESSES: the bf16-state route of the row-sharded UVd driver with the staged bf16 kernels on each rank's rows and
REAL collectives (the pattern of tests/test_sharded_2proc_gpu.py).  Transports:
  gloo-one-device   two ranks on cuda:0, gloo over device tensors
  rccl-two-devices  rank k on cuda:k over RCCL: runs where torch.cuda.device_count() >= 2, skipped otherwise
  rccl-one-rank     a 1-rank RCCL group on cuda:0 (the exchanges go through the library's own communicator)
N = 200003, r = 20.  The fused step on both branches: the stored state against the fp64 oracle on the global problem with the bars
of tests/test_uvd_bf16_gpu.py (every element within 2^-7 |y64| + 1e-5 rms(y64); share of codes that are neither floor nor ceil of
y64 <= 2 x that of the fp32 kernels + 1e-4), the gradient within 1e-5 of the oracle apply on the stored state, the r x r
coefficients identical on both ranks, 4 exchanges.  Then UVd(group=, state_route="native") for 4 steps (step 1 clips, step 2 leaves
the preconditioner alone, step 3 is finite-difference) and once more with step_tail="fused": per step 4 exchanges (2 on the step
without an update) + 1 collective when clipping; the state stays bfloat16 and finite and the coefficients agree across the ranks."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

from oracle import psgd_oracle as orc
from tests.uvd_cases import TINY32, check_bf16_state, make_uvd_problem, rel_err, to_bf16_np

pytestmark = pytest.mark.gpu
N, R, STEP, SEEDS = 200003, 20, 0.01, (11, 12)
CLS_SHAPES = [(300, 40), (5000,), (64, 64), (1000, 1), (1,)]
CLS_CLIP = [float("inf"), 0.05, float("inf"), float("inf")]
CLS_PROB = [1.0, 1.0, 0.0, 1.0]
CLS_EXACT = [True, True, True, False]


def _problem():
    p = make_uvd_problem(N, R, seed=21, uv_gain=2.0, d_spread=0.3)
    for k in ("U", "V", "d"):
        p[k] = to_bf16_np(p[k])
    return p


def _worker(rank, port, outdir, world, backend, two_devices):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    dev = torch.device("cuda", rank if two_devices else 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import preconditioned_stochastic_gradient_descent as psgd
    from psgd_tf_amd import sharded
    saved = {}
    # ---- functional: the fused step on both branches, row0 looked up (None)
    p = _problem()
    lo, hi = sharded.shard_rows(N, rank, world)
    t = {}
    for k, a in p.items():
        x = torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(dev)
        t[k] = x.to(torch.bfloat16) if k in ("U", "V", "d") else x
    be = sharded.hip_backend_for(t["U"])
    assert isinstance(be, sharded.HipStagesBf16)
    for i, upd in enumerate((True, False)):
        ex0 = sharded.EXCHANGES["count"]
        out = sharded.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32, balance=False,
                                                               update_U=upd, rounding="stochastic", rounding_seed=SEEDS[i])
        saved["ex%d" % i] = np.array(sharded.EXCHANGES["count"] - ex0)
        saved["co%d" % i] = be.coefficients().cpu().numpy().copy()
        saved["out%d" % i] = out.cpu().numpy()
        for k in ("U", "V", "d"):
            saved["%s%d" % (k, i)] = t[k].float().cpu().numpy()
    assert sharded.global_row0(hi - lo, dev, None) == lo
    # ---- class UVd, native state, row-sharded
    clips = {"n": 0}
    real = sharded.all_reduce_sum_f64_

    def counted(*a, **k):
        clips["n"] += 1
        return real(*a, **k)
    sharded.all_reduce_sum_f64_ = counted
    for tail in ("torch", "fused"):
        g = torch.Generator().manual_seed(91)
        params = [(torch.randn(s, generator=g) * 0.3).to(dev) for s in CLS_SHAPES]
        mine = slice(None) if world == 1 else (slice(0, 2) if rank == 0 else slice(2, None))
        own = [q.clone().requires_grad_(True) for q in params[mine]]
        opt = psgd.UVd(own, rank_of_modification=10, lr_params=0.004, lr_preconditioner=0.05,
                       generator=torch.Generator().manual_seed(606 + 13 * rank), group=dist.group.WORLD, state_dtype=torch.bfloat16,
                       state_route="native", step_tail=tail)
        assert opt._U.dtype == torch.bfloat16 and opt._U.shape[0] == sum(q.numel() for q in own)
        saved["seed0_" + tail] = np.array(opt._round_seed0)                      # one seed for all ranks (rank 0's generator)

        def loss():
            flat = torch.cat([q.reshape(-1) for q in own])
            w = torch.cos(torch.arange(flat.numel(), dtype=flat.dtype, device=dev) * 0.37 + rank)
            return 0.5 * torch.sum((1.0 + w * w) * flat * flat) + 0.25 * torch.sum(flat ** 4)
        counts = []
        for it in range(4 if tail == "torch" else 1):
            opt.grad_clip_max_norm.assign(CLS_CLIP[it] if tail == "torch" else 0.05)
            opt.preconditioner_update_probability.assign(CLS_PROB[it])
            opt.exact_hessian_vector_product.assign(CLS_EXACT[it])
            e0, c0 = sharded.EXCHANGES["count"], clips["n"]
            l = opt.step(loss)
            counts.append([sharded.EXCHANGES["count"] - e0, clips["n"] - c0])
            assert torch.isfinite(l.detach()).all()
        assert all(x.dtype == torch.bfloat16 and torch.isfinite(x.float()).all() for x in (opt._U, opt._V, opt._d))
        assert all(torch.isfinite(q).all() for q in own)
        saved["counts_" + tail] = np.array(counts)
        saved["cls_co_" + tail] = sharded.hip_backend_for(opt._U).coefficients().cpu().numpy().copy()
    saved["backend"] = np.array(dist.get_backend())
    np.savez(os.path.join(outdir, "r%d.npz" % rank), **saved)
    dist.barrier()
    dist.destroy_process_group()


def _two_devices():
    return torch.cuda.device_count() >= 2          # (counting devices does not initialise the GPU runtime)


@pytest.mark.parametrize("transport", [
    "gloo-one-device",
    pytest.param("rccl-two-devices", marks=pytest.mark.skipif(not _two_devices(), reason="needs two GPUs (rank k on cuda:k over RCCL)")),
    "rccl-one-rank"])
def test_bf16_state_sharded_real_kernels_real_collectives(hip_lib, transport):
    import torch.multiprocessing as mp
    import preconditioned_stochastic_gradient_descent as psgd
    outdir = tempfile.mkdtemp()
    port = 29000 + os.getpid() % 300
    world = 1 if transport == "rccl-one-rank" else 2
    backend = "gloo" if transport == "gloo-one-device" else "nccl"
    mp.start_processes(_worker, args=(port, outdir, world, backend, transport == "rccl-two-devices"), nprocs=world, join=True,
                       start_method="spawn")
    sh = [np.load(os.path.join(outdir, "r%d.npz" % k)) for k in range(world)]
    assert str(sh[0]["backend"]) == backend
    for s in sh:
        assert int(s["ex0"]) == 4 and int(s["ex1"]) == 4                       # stages 11, 12, 1, 2
        # per step: exchanges, clip collectives
        assert s["counts_torch"].tolist() == [[4, 0], [4, 1], [2, 0], [4, 0]], s["counts_torch"]
        assert s["counts_fused"].tolist() == [[4, 1]], s["counts_fused"]
    for k in ("co0", "co1", "cls_co_torch", "cls_co_fused", "seed0_torch", "seed0_fused"):
        assert all(s[k].tobytes() == sh[0][k].tobytes() for s in sh), k        # every rank redid the r x r algebra on the same numbers
    # the stored state and the gradient against the fp64 oracle on the global problem
    p = _problem()
    q = {k: v.astype(np.float64) for k, v in p.items()}
    w = {k: torch.from_numpy(v).cuda() for k, v in p.items()}
    for i, upd in enumerate((True, False)):
        orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], STEP, TINY32, balance=False, update_U=upd)
        psgd.update_precond_UVd_math_(w["U"], w["V"], w["d"], w["v"], w["h"], STEP, TINY32, balance=False, update_U=upd)
        stored = {k: np.concatenate([s["%s%d" % (k, i)] for s in sh], 0).astype(np.float64) for k in ("U", "V", "d")}
        tag = "%s fused step %d" % (transport, i)
        pn, pw, _ = check_bf16_state(tag, stored, {k: q[k] for k in ("U", "V", "d")}, {k: w[k].cpu().numpy() for k in ("U", "V", "d")},
                                     {"d", "U" if upd else "V"}, "stochastic")
        print("%s p_native=%.3e p_widen=%.3e" % (tag, pn, pw))
        assert pn <= 2 * pw + 1e-4, (tag, pn, pw)
        out = np.concatenate([s["out%d" % i] for s in sh], 0)
        e = rel_err(out, orc.precond_grad_UVd_math(stored["U"], stored["V"], stored["d"], q["g"]))
        assert e < 1e-5, (tag, e)
        # the next step starts from what was STORED (the oracle and the fp32 yardstick follow the bf16 state)
        for k in ("U", "V", "d"):
            q[k] = stored[k].copy()
            w[k] = torch.from_numpy(stored[k].astype(np.float32)).cuda()
