"""Sparse-LU preconditioner on a bf16-stored state: update + apply rounds beside an fp32 copy of the state (needs the MI355X).

The four factors live in HBM as bfloat16 -- (2r + 2) * 2 bytes per parameter instead of (2r + 2) * 4 -- and are read and
written by their own kernels (psgd_splu_bf16.hip); perturbations and gradients stay float32.  Every update rescales every
element (the balance of psgd.py:411-417), so every element is re-rounded each call: stochastic rounding keeps that unbiased.

    python examples/splu_bf16_update_apply.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

N, r, dev = 200_000, 10, torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)
psgd.manual_seed(0)                                        # the rounding seeds are drawn from the module's generator

# the shape of the state of demo_usage_of_all_preconditioners.py:47-51 (here Q = I), stored as bfloat16
L12 = torch.cat([torch.eye(r), torch.zeros(N - r, r)]).to(dev, torch.bfloat16)
U12 = torch.cat([torch.eye(r), torch.zeros(r, N - r)], 1).to(dev, torch.bfloat16)
l3 = torch.ones(N - r, 1, device=dev, dtype=torch.bfloat16)
u3 = torch.ones(N - r, 1, device=dev, dtype=torch.bfloat16)
state = (L12, l3, U12, u3)
print("state: %.1f MB in bfloat16 (float32: %.1f MB)" % (sum(t.numel() for t in state) * 2 / 1e6, sum(t.numel() for t in state) * 4 / 1e6))

# the same updates on an fp32 copy of the state: the bf16 state follows it to within its own precision (2^-9 per rounding)
ref = tuple(t.float() for t in state)
hess = torch.exp(torch.empty(N, 1, device=dev).uniform_(-1.0, 1.0, generator=gen))      # a diagonal Hessian
g = torch.randn(N, 1, device=dev, generator=gen)
for it in range(20):
    dx = torch.randn(N, 1, device=dev, generator=gen)
    state = psgd.update_precond_splu(*state, [dx], [hess * dx], 0.01, rounding="stochastic")
    ref = psgd.update_precond_splu(*ref, [dx], [hess * dx], 0.01)
    if it % 5 == 4:
        pg, pg_ref = psgd.precond_grad_splu(*state, [g])[0], psgd.precond_grad_splu(*ref, [g])[0]
        print("update %2d: |P g (bf16 state) - P g (fp32 state)| / |P g| = %.2e" % (it + 1, float((pg - pg_ref).norm() / pg_ref.norm())))
assert all(t.dtype == torch.bfloat16 for t in state) and pg.dtype == torch.float32
