"""Dense preconditioner on a small sparse tensor decomposition (the dense case of the reference's
demo_usage_of_all_preconditioners.py, written for torch): fit a rank-5 CP model x_r (x) y_r (x) z_r to a
random 10 x 20 x 50 tensor, with an L1 penalty of 1e-3 on the factors.  The three factor matrices hold
5 * (10 + 20 + 50) = 400 parameters, so Q is a 400 x 400 dense matrix: on a ROCm device in fp32 both
update_precond_dense and precond_grad_dense run in the HIP kernels of psgd_dense.hip.

    Q = 0.1 I,  update step 0.1,  learning rate 0.1,  Hessian-vector products by double backward (torch.autograd)

Every random draw (target, initial factors, the probe vectors v of every iteration) comes from one CPU generator,
so runs on different devices and dtypes see the same numbers.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

SHAPE, RANK = (10, 20, 50), 5


def loss_fn(target, factors):
    x, y, z = factors
    recon = torch.einsum("ri,rj,rk->ijk", x, y, z)
    err = target - recon
    return torch.sum(err * err) + 1e-3 * sum(torch.sum(torch.abs(w)) for w in factors)


def run(num_iter=200, seed=0, device="cuda", dtype=torch.float32, update=None, apply=None):
    """Returns the loss before each iteration and the final Q.  update / apply default to psgd's dense pair; any pair of
    functions with the same signatures (torch tensors in and out) can stand in."""
    update = update or psgd.update_precond_dense
    apply = apply or psgd.precond_grad_dense
    gen = torch.Generator().manual_seed(seed)
    put = lambda t: t.to(device=device, dtype=dtype)
    target = put(torch.rand(SHAPE, generator=gen, dtype=torch.float64))
    factors = [put(torch.randn((RANK, n), generator=gen, dtype=torch.float64)).requires_grad_() for n in SHAPE]
    num_para = sum(w.numel() for w in factors)
    Q = put(0.1 * torch.eye(num_para, dtype=torch.float64))
    losses = []
    for _ in range(num_iter):
        loss = loss_fn(target, factors)
        grads = torch.autograd.grad(loss, factors, create_graph=True)
        vs = [put(torch.randn(w.shape, generator=gen, dtype=torch.float64)) for w in factors]
        hess_vs = torch.autograd.grad(grads, factors, vs)
        losses.append(float(loss.detach()))
        Q = update(Q, vs, [h.detach() for h in hess_vs], step=0.1)
        pre_grads = apply(Q, [g.detach() for g in grads])
        with torch.no_grad():
            for w, g in zip(factors, pre_grads):
                w.sub_(0.1 * g)
    return losses, Q


if __name__ == "__main__":
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    losses, _ = run(device=dev)
    print("%s: loss %.4f -> %.4f over %d iterations" % (dev, losses[0], losses[-1], len(losses)))
