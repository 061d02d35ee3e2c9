"""examples/uvd_functional_step.py with the preconditioner state STORED in bf16 (psgd.py:671, :688-690 for a bf16 model): U, V, d
are bfloat16 tensors that the bf16-state kernels read and write themselves (psgd_uvd_bf16.hip) -- half the state memory, no fp32
copy at any time.  Stochastic rounding is what lets a bf16 d learn (its increments are below half a bf16 spacing); try `nearest`
to see the difference.

    python examples/uvd_functional_step_bf16.py [N] [r] [steps] [stochastic|nearest]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


def run(N=2_000_000, r=10, steps=200, rounding="stochastic", lr=0.5, seed=0, device="cuda:0"):
    """the least-squares toy problem of uvd_functional_step.py; returns the losses"""
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed(seed)
    c = torch.exp(torch.empty(N, 1, device=dev).uniform_(-2.3, 2.3, generator=g))
    x = torch.randn(N, 1, device=dev, generator=g)
    scale = (1.0 / (N * r)) ** 0.5                                                   # psgd.py:687
    U = (torch.randn(N, r, device=dev, generator=g) * scale).to(torch.bfloat16)      # :688
    V = (torch.randn(N, r, device=dev, generator=g) * scale).to(torch.bfloat16)      # :689
    d = torch.full((N, 1), 0.3, device=dev).to(torch.bfloat16)                       # :690
    gen = torch.Generator().manual_seed(seed)          # the coins of :562, :588 and the rounding seeds
    losses = []
    for _ in range(steps):
        losses.append(float(0.5 * torch.sum(c * x * x)))
        grad = c * x
        v = torch.randn(N, 1, device=dev, generator=g)
        h = c * v
        pre = psgd.update_precond_UVd_math_and_precond_grad(U, V, d, v, h, grad, 0.1, psgd._tiny, generator=gen, rounding=rounding)
        x = x - lr * pre
    losses.append(float(0.5 * torch.sum(c * x * x)))
    return losses


if __name__ == "__main__":
    a = sys.argv[1:]
    losses = run(int(a[0]) if a else 2_000_000, int(a[1]) if len(a) > 1 else 10, int(a[2]) if len(a) > 2 else 200,
                 a[3] if len(a) > 3 else "stochastic")
    print("bf16 state: loss %.4g -> %.4g in %d steps" % (losses[0], losses[-1], len(losses) - 1))
