"""Checkpoint and resume of class UVd ("Checkpoints"): a run interrupted half way, saved with torch.save, loaded
into a NEW optimizer and continued ends on the same bits as the uninterrupted run; the same fp32 checkpoint then continues on the
native bf16 route (half the state memory), narrowed on load by psgd_uvd_bf16_narrow_f32 through a bounded staging buffer; and a
checkpoint is split into two row shards and joined again offline.

    python examples/uvd_checkpoint_resume.py [N] [r] [steps]
"""
import io
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402
from psgd_tf_amd import sharded  # noqa: E402


def problem(N, device, seed=0):
    g = torch.Generator(device=device).manual_seed(seed)
    c = torch.exp(torch.empty(N, device=device).uniform_(-2.3, 2.3, generator=g))
    w0 = torch.randn(N, device=device, generator=g)
    return c, w0


def optimizer(w, r, seed, **kw):
    return psgd.UVd([w], rank_of_modification=r, lr_params=0.2, lr_preconditioner=0.1, preconditioner_update_probability=0.5,
                    generator=torch.Generator().manual_seed(seed), **kw)


def run(N=1_000_000, r=10, steps=40, device="cuda:0"):
    dev = torch.device(device)
    c, w0 = problem(N, dev)
    half = steps // 2

    def go(opt, w, ks):
        for _ in ks:
            loss = opt.step(lambda: 0.5 * torch.sum(c * w * w))
        return float(loss.detach())

    # the uninterrupted run
    torch.cuda.manual_seed(1)
    w = w0.clone().requires_grad_(True)
    want = go(optimizer(w, r, seed=3), w, range(steps))
    w_want = w.detach().clone()

    # the same run, saved half way ...
    torch.cuda.manual_seed(1)
    w = w0.clone().requires_grad_(True)
    opt = optimizer(w, r, seed=3)
    go(opt, w, range(half))
    buf = io.BytesIO()
    torch.save({"uvd": opt.state_dict(), "w": w.detach().cpu(), "cuda_rng": torch.cuda.get_rng_state(dev)}, buf)

    # ... and continued by a new process' worth of objects: another generator seed, the load replaces it
    buf.seek(0)
    ckpt = torch.load(buf, weights_only=True)
    w = ckpt["w"].to(dev).requires_grad_(True)
    opt = optimizer(w, r, seed=12345)
    opt.load_state_dict(ckpt["uvd"])
    torch.cuda.set_rng_state(ckpt["cuda_rng"], dev)          # the probe vectors' generator is the caller's to restore
    got = go(opt, w, range(half, steps))
    print("resumed: loss %.6g, uninterrupted %.6g, parameters bit-identical: %s" % (got, want, torch.equal(w.detach(), w_want)))

    # the fp32 checkpoint continued on the native bf16 route: no fp32 copy of the state on the device beyond the staging buffer
    w = ckpt["w"].to(dev).requires_grad_(True)
    opt = optimizer(w, r, seed=12345, state_dtype=torch.bfloat16, state_route="native")
    opt.load_state_dict(ckpt["uvd"])
    torch.cuda.set_rng_state(ckpt["cuda_rng"], dev)
    print("fp32 checkpoint -> native bf16 state (%s): loss %.6g" % (opt._U.dtype, go(opt, w, range(half, steps))))

    # offline: the checkpoint as two row shards, and back
    cut = (N // 2 + 63) // 64 * 64
    two = sharded.reshard_uvd_state([ckpt["uvd"]], [cut, N - cut])
    one = sharded.reshard_uvd_state(two, [N])[0]
    print("resharded 1 -> 2 -> 1: rows %s, identical: %s" % ([s["num_params"] for s in two], torch.equal(one["U"], ckpt["uvd"]["U"])))
    return got, want


if __name__ == "__main__":
    a = sys.argv[1:]
    run(int(a[0]) if a else 1_000_000, int(a[1]) if len(a) > 1 else 10, int(a[2]) if len(a) > 2 else 40)
