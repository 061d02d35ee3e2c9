"""class UVd on a ROW-SHARDED flat parameter vector with the preconditioner state stored in bf16 and handled by the bf16-state kernels
themselves (state_route="native"): this rank's rows of U, V, d are bfloat16 tensors, no fp32 copy of them exists at any time, and a
step costs four small exchanges (the Gram, max|nablaD|, and the two r-vectors of the apply).  Here the group has ONE rank, so the
example runs on one GPU; with one process per GPU (torchrun) every rank passes its own parameters and the same code runs unchanged.

    python examples/uvd_sharded_bf16_step.py [N] [steps]
"""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402
from psgd_tf_amd import sharded  # noqa: E402


def run(N=1_000_000, steps=100, device="cuda:0"):
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    own_group = not dist.is_initialized()
    if own_group:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29544")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)       # "nccl" is RCCL on ROCm
    try:
        g = torch.Generator(device=dev).manual_seed(0)
        c = torch.exp(torch.empty(N, device=dev).uniform_(-2.3, 2.3, generator=g))
        w = torch.randn(N, device=dev, generator=g).requires_grad_(True)            # THIS rank's parameters
        opt = psgd.UVd([w], rank_of_modification=10, lr_params=0.5, lr_preconditioner=0.1, generator=torch.Generator().manual_seed(0),
                       group=dist.group.WORLD, state_dtype=torch.bfloat16, state_route="native")
        assert opt._U.dtype == opt._V.dtype == opt._d.dtype == torch.bfloat16
        losses = []
        e0 = sharded.EXCHANGES["count"]
        for _ in range(steps):
            losses.append(float(opt.step(lambda: 0.5 * torch.sum(c * w * w))))
        return losses, (sharded.EXCHANGES["count"] - e0) / steps
    finally:
        if own_group:
            dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv[1:]
    losses, per_step = run(int(a[0]) if a else 1_000_000, int(a[1]) if len(a) > 1 else 100)
    print("sharded bf16 state (1-rank group): loss %.4g -> %.4g in %d steps, %.0f exchanges per step" % (losses[0], losses[-1], len(losses), per_step))
