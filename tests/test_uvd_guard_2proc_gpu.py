"""GPU, two PROCESSES on one device (gloo over device tensors, spawned as tests/test_uvd_bf16_sharded_2proc_gpu.py spawns its own):
the guarded step of a row-sharded UVd.  A non-finite gradient is owned by rank 1 ALONE; both ranks skip that step, both ranks'
shards keep their bits, both ranks then take a good step, and a guarded step costs the collectives of an unguarded one plus one
(the MAX over the ranks' verdicts) on both ranks -- counted with a spy on the collective helpers of psgd_tf_amd.sharded.  On the
fp32 route and on the native bf16 route, with both tails."""
import math
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = [(300, 40), (5000,), (64, 64), (1000, 1), (1,)]
ROUTES = {"fp32": {}, "bf16-native": dict(state_dtype=torch.bfloat16, state_route="native")}


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy().copy()


def _worker(rank, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import preconditioned_stochastic_gradient_descent as psgd
    from psgd_tf_amd import sharded
    n = {"clip": 0, "max": 0}
    real_sum, real_max = sharded.all_reduce_sum_f64_, sharded.all_reduce_max_i32_

    def counted_sum(*a, **k):
        n["clip"] += 1
        return real_sum(*a, **k)

    def counted_max(*a, **k):
        n["max"] += 1
        return real_max(*a, **k)
    sharded.all_reduce_sum_f64_, sharded.all_reduce_max_i32_ = counted_sum, counted_max
    collectives = lambda: sharded.EXCHANGES["count"] + n["clip"] + n["max"]
    saved = {}
    for route, rkw in ROUTES.items():
        for tail in ("fused", "torch"):
            tag = "%s_%s" % (route, tail)
            counts = {}
            for nonfinite in ("propagate", "skip"):
                g = torch.Generator().manual_seed(91)
                params = [(torch.randn(s, generator=g) * 0.3).to(dev) for s in SHAPES]
                own = [q.clone().requires_grad_(True) for q in params[slice(0, 2) if rank == 0 else slice(2, None)]]
                torch.manual_seed(50 + rank)
                opt = psgd.UVd(own, rank_of_modification=10, lr_params=0.004, lr_preconditioner=0.05, grad_clip_max_norm=0.05,
                               momentum=0.9, generator=torch.Generator().manual_seed(606 + 13 * rank), group=dist.group.WORLD,
                               step_tail=tail, nonfinite=nonfinite, **rkw)
                factor = {"x": 1.0}

                def loss():
                    flat = torch.cat([q.reshape(-1) for q in own])
                    w = torch.cos(torch.arange(flat.numel(), dtype=flat.dtype, device=dev) * 0.37 + rank)
                    return (0.5 * torch.sum((1.0 + w * w) * flat * flat) + 0.25 * torch.sum(flat ** 4)) * factor["x"]
                c0 = collectives()
                opt.step(loss)
                counts[nonfinite] = collectives() - c0
                if nonfinite == "propagate":
                    continue
                before = [_bits(t) for t in own + [opt._U, opt._V, opt._d, opt._momentum_buffer()]]
                k0 = (opt._m_step, getattr(opt, "_round_step", None))
                factor["x"] = math.inf if rank == 1 else 1.0                 # rank 0's own gradient is finite
                c0 = collectives()
                ret = opt.step(loss)
                saved[tag + "_bad_collectives"] = np.array(collectives() - c0)
                factor["x"] = 1.0
                assert math.isfinite(float(ret)) == (rank == 0)
                after = [_bits(t) for t in own + [opt._U, opt._V, opt._d, opt._momentum_buffer()]]
                saved[tag + "_skipped"] = np.array([int(opt.last_step_skipped), opt.skipped_steps])
                saved[tag + "_kept"] = np.array(all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
                                                and k0 == (opt._m_step, getattr(opt, "_round_step", None)))
                c0 = collectives()
                opt.step(loss)
                saved[tag + "_good"] = np.array([int(opt.last_step_skipped), opt.skipped_steps, collectives() - c0,
                                                 int(all(bool(torch.isfinite(t.float()).all()) for t in own + [opt._U, opt._V, opt._d]))])
                saved[tag + "_moved"] = np.array(any(a.tobytes() != _bits(t).tobytes() for a, t in zip(after, own)))
            saved[tag + "_counts"] = np.array([counts["propagate"], counts["skip"]])
    np.savez(os.path.join(outdir, "r%d.npz" % rank), **saved)
    dist.barrier()
    dist.destroy_process_group()


def test_rank_divergent_overflow_skips_on_both_ranks(hip_lib):
    import torch.multiprocessing as mp
    outdir = tempfile.mkdtemp()
    port = 29300 + os.getpid() % 300
    mp.start_processes(_worker, args=(port, outdir), nprocs=2, join=True, start_method="spawn")
    sh = [np.load(os.path.join(outdir, "r%d.npz" % k)) for k in range(2)]
    for route in ROUTES:
        for tail in ("fused", "torch"):
            tag = "%s_%s" % (route, tail)
            exchanges = 4 if route == "bf16-native" else 2
            for rank, s in enumerate(sh):
                what = (tag, rank)
                assert s[tag + "_counts"].tolist() == [exchanges + 1, exchanges + 2], (what, s[tag + "_counts"])    # + clip, + verdict
                assert s[tag + "_skipped"].tolist() == [1, 1], what                 # both ranks skipped, rank 0 on rank 1's word
                assert int(s[tag + "_bad_collectives"]) == 1, what                  # the verdict alone: no exchange, no clip norm
                assert bool(s[tag + "_kept"]), what
                assert s[tag + "_good"].tolist() == [0, 1, exchanges + 2, 1], (what, s[tag + "_good"])
                assert bool(s[tag + "_moved"]), what
