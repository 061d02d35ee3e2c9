"""class SPLU on the reference's demo problem (demo_usage_of_all_preconditioners.py, the sparse LU case, written for torch): fit
a rank-5 CP model x_r (x) y_r (x) z_r to a random 10 x 20 x 50 tensor with an L1 penalty of 1e-3 on the factors -- 400
parameters in three tensors, a preconditioner of order r = 10.

The demo's hand-written step (:46-62) becomes three lines: the constructor's defaults for the initial scale (0.1) and the
preconditioner step (0.1) are the demo's, the learning rate is its 0.1, Hessian-vector products come from a double backward.

    python examples/splu_class.py [fused|torch]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

SHAPE, RANK = (10, 20, 50), 5


def main(steps=100, step_tail="fused", seed=0, quiet=False, **kw):
    """Returns the loss before each step.  kw: further arguments of psgd.SPLU."""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(seed)
    target = torch.rand(SHAPE, generator=gen).to(dev)
    xyz = [torch.randn((RANK, n), generator=gen).to(dev).requires_grad_() for n in SHAPE]
    torch.manual_seed(seed)                                            # the probe vectors of the step come from the global generator

    def closure():
        err = target - torch.einsum("ri,rj,rk->ijk", *xyz)
        return torch.sum(err * err) + 1e-3 * sum(torch.sum(torch.abs(w)) for w in xyz)

    opt = psgd.SPLU(xyz, rank_of_modification=10, lr_params=0.1, step_tail=step_tail, generator=torch.Generator().manual_seed(seed), **kw)
    losses = []
    for k in range(steps):
        losses.append(float(opt.step(closure).detach()))
        if not quiet and k % 10 == 0:
            print("step %3d  loss %.4f" % (k, losses[-1]))
    if not quiet:
        print("loss %.4f -> %.4f over %d steps: a factor of %.3g" % (losses[0], losses[-1], steps, losses[0] / losses[-1]))
    return losses


if __name__ == "__main__":
    main(step_tail=sys.argv[1] if len(sys.argv) > 1 else "fused")
