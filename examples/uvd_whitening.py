"""class UVd with preconditioner_fit="whitening": a model whose backward cannot be differentiated twice.

A two-layer regression net whose loss head is a custom autograd.Function marked once_differentiable -- the stand-in for a fused
loss or attention kernel, or a vendor op, whose backward is itself a kernel.  The Hessian fit needs the loss differentiated twice:
on the exact route step() runs autograd.grad(..., create_graph=True) and then differentiates those gradients again, and the
gradients that come out of such a Function have no graph to differentiate (the RuntimeError is caught and printed below).  The
whitening fit feeds the same preconditioner update the pair (v, g), v ~ N(0, I) drawn into the flat vector by ONE multi_randn
launch per step, so a step is one ordinary backward pass.

    python examples/uvd_whitening.py [steps]

The whitened gradient has roughly unit scale per element, as Adam's update has: lr_params is chosen for it here and would be far
too large for the Hessian fit.
"""
import os
import sys

import torch
from torch.autograd.function import once_differentiable

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


class FusedMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, target):
        diff = out - target
        ctx.save_for_backward(diff)
        return torch.mean(diff * diff)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (diff,) = ctx.saved_tensors
        return g * diff * (2.0 / diff.numel()), None


def model(dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(256, 32, device=dev, generator=gen)
    y = torch.sin(x @ torch.randn(32, 4, device=dev, generator=gen))
    params = [(0.2 * torch.randn(s, device=dev, generator=gen)).requires_grad_(True) for s in ((32, 64), (64,), (64, 4), (4,))]
    W1, b1, W2, b2 = params

    def closure():
        return FusedMSE.apply(torch.tanh(x @ W1 + b1) @ W2 + b2, y)
    return params, closure


def main(steps=200):
    dev = torch.device("cuda:0")
    kw = dict(rank_of_modification=10, lr_params=0.02, lr_preconditioner=0.1, step_tail="fused",
              generator=torch.Generator().manual_seed(1))
    params, closure = model(dev)
    opt = psgd.UVd(params, exact_hessian_vector_product=True, **kw)
    error = None
    try:
        opt.step(closure)
    except RuntimeError as e:
        error = str(e).splitlines()[0]
    print("preconditioner_fit='hessian', exact products: RuntimeError: %s" % error)

    params, closure = model(dev)
    opt = psgd.UVd(params, preconditioner_fit="whitening", probe_seed=2, **kw)
    first = float(closure().detach())
    for _ in range(steps):
        opt.step(closure)
    last = float(closure().detach())
    print("preconditioner_fit='whitening': loss %.4e -> %.4e after %d steps (%d probes drawn)" % (first, last, steps, opt.probe_step))
    return error, first, last


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
