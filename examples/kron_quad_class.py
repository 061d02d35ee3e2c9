"""class Kron with preconditioner_update="quad": the inverse-free whitening update on symmetric factors.

A two-layer regression whose gradients are badly scaled (the inputs' columns span 1e-2 .. 1e2).  The (dense, dense) matrix
layers run update_precond_kron_quad_ / precond_grad_kron_quad (products and norms only: no triangular solve, no inverse, no
probe); the bias vector keeps the triangular whitening update.  The same model is trained with the default triangular update
for comparison.  At the fixed point of the definition P = Ql Ql (x) Qr Qr is the INVERSE of the gradient's Kronecker covariance
(include/psgd_kron_quad_hip.h), so the preconditioned gradient grows as the gradient shrinks: the step is bounded here with
grad_clip_max_norm, and an lr_params tuned for the triangular whitening fit does not carry over.

    python examples/kron_quad_class.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


def model(dev):
    gen = torch.Generator().manual_seed(0)
    X = (torch.randn(256, 48, generator=gen) * torch.logspace(-2, 2, 48)).to(dev)
    Y = torch.tanh(X @ (torch.randn(48, 24, generator=gen) / torch.logspace(-2, 2, 48)[:, None]).to(dev))
    params = [(torch.randn(48, 32, generator=gen) * 0.01).to(dev).requires_grad_(), torch.zeros(32, device=dev, requires_grad=True),
              (torch.randn(32, 24, generator=gen) * 0.1).to(dev).requires_grad_()]

    def closure():
        W1, b1, W2 = params
        return ((torch.tanh(X @ W1 + b1) @ W2 - Y) ** 2).mean()
    return params, closure


def main(steps=300):
    assert torch.cuda.is_available(), "this example runs on the HIP device"
    dev = torch.device("cuda:0")
    for update in ("triangular", "quad"):
        params, closure = model(dev)
        opt = psgd.Kron(params, "dense", 1.0, 0.01, 0.1, 1.0, any_rank=True, preconditioner_fit="whitening", probe_seed=2,
                        generator=torch.Generator().manual_seed(1), preconditioner_update=update)
        first = float(closure().detach())
        for _ in range(steps):
            opt.step(closure)
        print("preconditioner_update=%r: loss %.4e -> %.4e after %d steps; quad layers %s"
              % (update, first, float(closure().detach()), steps, opt.quad_layers))
        for i in opt.quad_layers:
            Ql, Qr = opt.factors[i]
            print("  layer %d: L = %s, factors symmetric: %s" % (i, opt.quad_L[i].tolist(), bool(torch.equal(Ql, Ql.T) and torch.equal(Qr, Qr.T))))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 300)
