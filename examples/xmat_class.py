"""class XMat, the O(N) X-shaped preconditioner, on two small problems on the device.

train      a 3-tensor least-squares problem with per-coordinate curvature spread over four decades: psgd.XMat(params) and
           opt.step(closure), the class name swapped in where psgd.UVd stood.  diagonal=True is the diagonal preconditioner.
whiten     the gradient-whitening fit on a 256-element quadratic with curvature 0.01 .. 100: the gradient of every step is
           c * N(0, 1) (a fresh target per step, the parameters held still by lr_params = 0), so sigma_g = c and a whitening
           preconditioner brings diag(Q'Q) * sigma_g to 1 in every coordinate.  Returns that vector and, per step, (v, h).

    python examples/xmat_class.py [fused|torch]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


def train(steps=200, step_tail="fused", seed=0, quiet=False, **kw):
    """Returns the loss before each step.  kw: further arguments of psgd.XMat."""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(seed)
    shapes = [(16, 8), (33,), (4, 5, 3)]
    params = [torch.randn(s, generator=gen).to(dev).requires_grad_() for s in shapes]
    curv = [torch.exp(torch.empty(s).uniform_(-4.6, 4.6, generator=gen)).to(dev) for s in shapes]
    torch.manual_seed(seed)                                            # the probe vectors of the step come from the global generator

    def closure():
        return sum(0.5 * torch.sum(c * p * p) for c, p in zip(curv, params))

    opt = psgd.XMat(params, preconditioner_init_scale=0.05, lr_params=0.2, lr_preconditioner=0.1, step_tail=step_tail, generator=torch.Generator().manual_seed(seed), **kw)
    losses = [float(opt.step(closure).detach()) for _ in range(steps)]
    if not quiet:
        print("train%s: loss %.4e -> %.4e over %d steps" % (" (diagonal)" if kw.get("diagonal") else "", losses[0], losses[-1], steps))
    return losses


def whiten(steps=500, n=256, step_tail="fused", on_step=None, **kw):
    """Returns (diag(Q'Q) * sigma_g, the optimizer).  on_step(opt): called after every step (a test reads v and h there)."""
    dev = torch.device("cuda:0")
    c = torch.logspace(-2, 2, n, device=dev)
    x = torch.zeros(n, device=dev, requires_grad=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    opt = psgd.XMat([x], lr_params=0.0, lr_preconditioner=0.1, step_tail=step_tail, preconditioner_fit="whitening", probe_seed=7,
                    generator=torch.Generator().manual_seed(0), **kw)
    for _ in range(steps):
        target = torch.randn(n, device=dev, generator=gen)
        opt.step(lambda: 0.5 * torch.sum(c * (x - target) ** 2))
        if on_step is not None:
            on_step(opt)
    b = torch.zeros_like(opt.a) if opt.b is None else opt.b
    return (opt.a ** 2 + torch.flip(b, [0]) ** 2) * c, opt


if __name__ == "__main__":
    tail = sys.argv[1] if len(sys.argv) > 1 else "fused"
    train(step_tail=tail)
    train(step_tail=tail, diagonal=True)
    w, _ = whiten(step_tail=tail)
    print("whiten: diag(Q'Q) * sigma_g in [%.3f, %.3f] after 500 steps (1 = whitened)" % (float(w.min()), float(w.max())))
