"""class Dense on the two problems the reference runs its dense preconditioner on, both on the device.

rosenbrock   hello_psgd.py:7-27: two scalar parameters at (-1, 1), Q = 0.1 I, 500 iterations with preconditioner step 0.2 and
             learning rate 0.5.  The loop of examples/hello_psgd.py (two function calls and the update, on the CPU) becomes a
             constructor and opt.step(closure); the 2 x 2 factor lives on the device and the kernels of psgd_dense.hip run it.
decompose    the dense case of demo_usage_of_all_preconditioners.py:26-41 (examples/tensor_decomposition_dense.py writes it with
             the two functions): a rank-5 CP model of a random 10 x 20 x 50 tensor with an L1 penalty of 1e-3 -- 400 parameters in
             three tensors, Q is 400 x 400; the constructor's defaults for the initial scale (0.1) and the preconditioner step
             (0.1) are the demo's, the learning rate is its 0.1.  The first steps only: this is a usage example.

    python examples/dense_class.py [fused|torch]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

SHAPE, RANK = (10, 20, 50), 5


def rosenbrock(steps=500, step_tail="fused", seed=0, quiet=False, **kw):
    """Returns (the loss before each step, the final (x1, x2), the final Q).  kw: further arguments of psgd.Dense."""
    dev = torch.device("cuda:0")
    xs = [torch.tensor(-1.0, device=dev, requires_grad=True), torch.tensor(1.0, device=dev, requires_grad=True)]      # :7
    torch.manual_seed(seed)                                            # the probe vectors of the step come from the global generator

    def closure():                                                     # :10-12
        x1, x2 = xs
        return 100.0 * (x2 - x1 ** 2) ** 2 + (1.0 - x1) ** 2

    opt = psgd.Dense(xs, preconditioner_init_scale=0.1, lr_params=0.5, lr_preconditioner=0.2, step_tail=step_tail, **kw)   # :8, :25, :27
    f = [opt.step(closure).detach() for _ in range(steps)]
    f, xs = torch.stack(f).cpu().tolist(), [float(x.detach()) for x in xs]
    if not quiet:
        print("rosenbrock: f %.3e -> %.3e after %d steps; x = (%.6f, %.6f)" % (f[0], f[-1], steps, xs[0], xs[1]))
    return f, xs, opt.Q.clone()                                        # (a clone: the tensor behind opt.Q alternates between two buffers)


def decompose(steps=20, step_tail="fused", seed=0, quiet=False, **kw):
    """Returns the loss before each step.  kw: further arguments of psgd.Dense."""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(seed)
    target = torch.rand(SHAPE, generator=gen).to(dev)
    xyz = [torch.randn((RANK, n), generator=gen).to(dev).requires_grad_() for n in SHAPE]
    torch.manual_seed(seed)

    def closure():
        err = target - torch.einsum("ri,rj,rk->ijk", *xyz)
        return torch.sum(err * err) + 1e-3 * sum(torch.sum(torch.abs(w)) for w in xyz)

    opt = psgd.Dense(xyz, lr_params=0.1, step_tail=step_tail, generator=torch.Generator().manual_seed(seed), **kw)
    losses = []
    for k in range(steps):
        losses.append(float(opt.step(closure).detach()))
        if not quiet and k % 5 == 0:
            print("decompose: step %3d  loss %.4f" % (k, losses[-1]))
    if not quiet:
        print("decompose: loss %.4f -> %.4f over %d steps" % (losses[0], losses[-1], steps))
    return losses


if __name__ == "__main__":
    tail = sys.argv[1] if len(sys.argv) > 1 else "fused"
    rosenbrock(step_tail=tail)
    decompose(step_tail=tail)
