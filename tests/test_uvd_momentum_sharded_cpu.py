"""class UVd with momentum and weight decay, row-sharded over a gloo group of two CPU processes (the stage doubles of
tests/cpu_stages.py): the momentum buffer is this rank's rows and needs no collective of its own.

  * every rank's buffer equals, bit for bit, the float32 recursion m <- fl(fl(beta_k m) + fl((1 - beta_k) g)) over the gradients
    that rank's closure gave (recomputed outside the optimizer from the parameters before each step);
  * the two ranks' buffers (and parameters) concatenated equal those of ONE rank that owns every parameter.  Bound: both are
    float32 realisations of the same recursion whose only difference is the fold order of the r-dimensional exchanges; the
    existing sharded class test holds each such run within 2e-5 (relative, five steps) of the fp64 oracle, so two of them are
    within 4e-5 of each other;
  * the collectives per step are those of a run without momentum: 2 exchanges, plus one scalar all-reduce when clipping;
  * state_dict() carries the rows, sharded.reshard_uvd_state moves them 2 -> 3 -> 1 ranks unchanged."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.uvd_cases import rel_err

SHAPES = [(3, 5), (7,), (64, 2), (6, 1), (1,)]                # rank 0 owns the first three tensors (150 rows)
SPLIT, R, STEPS = 3, 3, 5
MOM, WD = 0.7, 0.05


def _setup():
    g = torch.Generator().manual_seed(177)
    params = [torch.randn(s, generator=g) * 0.7 for s in SHAPES]
    n = sum(p.numel() for p in params)
    sc = (1.0 / (n * R)) ** 0.5
    U, V = torch.randn(n, R, generator=g) * sc * 6, torch.randn(n, R, generator=g) * sc * 6
    d = torch.exp(torch.randn(n, 1, generator=g) * 0.2)
    probes = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(STEPS)]
    return params, U, V, d, probes


def _loss(ps, salt):
    flat = torch.cat([p.reshape(-1) for p in ps])
    w = torch.cos(torch.arange(flat.numel(), dtype=flat.dtype) * 0.37 + salt)
    return 0.5 * torch.sum((1.0 + w * w) * flat * flat) + 0.25 * torch.sum(flat ** 4)


def _schedule(opt, it):
    opt.grad_clip_max_norm.assign([0.05, float("inf"), 0.05, 0.05, float("inf")][it])
    opt.exact_hessian_vector_product.assign([True, True, False, True, False][it])
    opt.preconditioner_update_probability.assign([1.0, 1.0, 1.0, 0.0, 1.0][it])


def _worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import preconditioned_stochastic_gradient_descent as psgd
        from psgd_tf_amd import preconditioned_stochastic_gradient_descent as prod
        from tests.cpu_stages import NumpyStages
        params, U, V, d, probes = _setup()
        if world == 1:
            mine = slice(0, None)
        else:
            mine = slice(0, SPLIT) if rank == 0 else slice(SPLIT, None)
        own = [p.clone().requires_grad_(True) for p in params[mine]]
        lo = sum(p.numel() for p in params[:mine.start or 0])
        hi = lo + sum(p.numel() for p in own)

        def loss():                                       # the global loss is the sum of the two halves' losses: block-diagonal
            if world == 1:
                return _loss(own[:SPLIT], 0.0) + _loss(own[SPLIT:], 1.0)
            return _loss(own, float(rank))
        opt = psgd.UVd(own, rank_of_modification=R, lr_params=0.004, lr_preconditioner=0.1, generator=torch.Generator().manual_seed(4321),
                       group=dist.group.WORLD, stage_backend=NumpyStages(R, dtype=np.float32), momentum=MOM, weight_decay=WD)
        opt._U.copy_(U[lo:hi]); opt._V.copy_(V[lo:hi]); opt._d.copy_(d[lo:hi])
        calls = {"all_gather_into_tensor": 0, "all_reduce": 0, "broadcast": 0}
        for name in calls:
            def wrap(fn, name=name):
                def counted(*a, **k):
                    calls[name] += 1
                    return fn(*a, **k)
                return counted
            setattr(dist, name, wrap(getattr(dist, name)))
        m_ref = np.zeros(hi - lo, dtype=np.float32)
        per_step = []
        for it in range(STEPS):
            queue = {id(p): q for p, q in zip(own, probes[it][mine])}
            prod._randn_like = lambda p: queue[id(p)].clone()
            _schedule(opt, it)
            g = np.concatenate([x.reshape(-1).numpy() for x in torch.autograd.grad(loss(), own)]).astype(np.float32)
            beta, omb = prod.uvd_momentum_coefficients(it, MOM)
            assert beta == float(np.float32(min(it / (it + 1.0), MOM)))
            m_ref = (np.float32(beta) * m_ref).astype(np.float32) + (np.float32(omb) * g).astype(np.float32)
            before = dict(calls)
            opt.step(loss)
            per_step.append({k: calls[k] - before[k] for k in calls})
            assert opt._m_step == it + 1
            assert np.array_equal(opt._m.numpy().view(np.int32), m_ref.view(np.int32)), (rank, it)
        clip = [True, False, True, True, False]
        for it, c in enumerate(per_step):
            assert c == {"all_gather_into_tensor": 2, "all_reduce": int(clip[it]), "broadcast": 0}, (it, c)
        sd = opt.state_dict()
        assert sd["momentum_step"] == STEPS and sd["row0"] == lo and sd["hyper"]["momentum"] == MOM and sd["hyper"]["weight_decay"] == WD
        assert torch.equal(sd["momentum_buffer"], opt._m) and sd["momentum_buffer"].data_ptr() != opt._m.data_ptr()
        torch.save(sd, os.path.join(outdir, "sd_w%d_r%d.pt" % (world, rank)))
        np.savez(os.path.join(outdir, "w%d_r%d.npz" % (world, rank)), m=opt._m.numpy(),
                 p=torch.cat([p.detach().reshape(-1) for p in own]).numpy())
    finally:
        dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_two_ranks_momentum_equals_one_rank_and_reshards():
    from psgd_tf_amd import sharded
    with tempfile.TemporaryDirectory() as outdir:
        mp.spawn(_worker, args=(2, _free_port(), outdir), nprocs=2, join=True)
        mp.spawn(_worker, args=(1, _free_port(), outdir), nprocs=1, join=True)
        two = [np.load(os.path.join(outdir, "w2_r%d.npz" % k)) for k in range(2)]
        one = np.load(os.path.join(outdir, "w1_r0.npz"))
        sds = [torch.load(os.path.join(outdir, "sd_w2_r%d.pt" % k), weights_only=True) for k in range(2)]
    m2, p2 = (np.concatenate([s[k] for s in two]) for k in ("m", "p"))
    n = sum(int(np.prod(s)) for s in SHAPES)
    assert m2.shape == (n,) and one["m"].shape == (n,) and np.isfinite(m2).all() and float(np.abs(m2).max()) > 1e-3
    print("two ranks vs one: m rel %.3g, parameters rel %.3g" % (rel_err(m2, one["m"]), rel_err(p2, one["p"])))
    assert rel_err(m2, one["m"]) < 4e-5
    assert rel_err(p2, one["p"]) < 4e-5
    # 2 -> 3 -> 1 ranks: the rows travel unchanged
    three = sharded.reshard_uvd_state(sds, [64, 64, n - 128])
    assert [int(s["momentum_buffer"].numel()) for s in three] == [64, 64, n - 128]
    whole = sharded.reshard_uvd_state(three, [n])[0]
    assert np.array_equal(whole["momentum_buffer"].numpy().view(np.int32), m2.view(np.int32))
    assert whole["momentum_step"] == STEPS and whole["hyper"]["momentum"] == MOM and whole["row0"] == 0
