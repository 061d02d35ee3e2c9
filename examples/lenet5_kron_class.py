"""class Kron on the LeNet5 weight shapes of the reference's mnist_with_lenet5.py (:12-16): the train_step of :43-57 as one
`opt.step(closure)`, with the per-tensor torch tail and with the fused multi-tensor tail.

Synthetic data: there is no MNIST here.  The loss is the quadratic sum_k tr(W_k' Hl_k W_k Hr_k) / 2 with the fixed SPD Hl, Hr of
examples/lenet5_kron_step.py; its gradient Hl W Hr and its Hessian-vector products come from autograd, as they would for LeNet5.

    python examples/lenet5_kron_class.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

SHAPES = [(26, 6), (151, 16), (257, 120), (121, 84), (85, 10)]          # W1 .. W5 of mnist_with_lenet5.py:12-16


def main(steps=200):
    dev = torch.device("cuda:0")
    out = {}
    for tail in ("torch", "fused"):
        g = torch.Generator(device=dev).manual_seed(0)
        Hl = [torch.diag(torch.exp(torch.empty(m, device=dev).uniform_(-1.5, 1.5, generator=g))) for m, n in SHAPES]
        Hr = [torch.diag(torch.exp(torch.empty(n, device=dev).uniform_(-1.5, 1.5, generator=g))) for m, n in SHAPES]
        Ws = [torch.randn(m, n, device=dev, generator=g).requires_grad_(True) for m, n in SHAPES]
        clip = 0.1 * sum(W.numel() for W in Ws) ** 0.5                                              # :63
        opt = psgd.Kron(Ws, "dense", lr_params=0.1, lr_preconditioner=0.1, grad_clip_max_norm=clip, step_tail=tail, generator=g)

        def closure():
            return sum(0.5 * torch.sum(W * (hl @ W @ hr)) for W, hl, hr in zip(Ws, Hl, Hr))
        first = float(closure().detach())
        for _ in range(steps):
            opt.step(closure)
        out[tail] = (first, float(closure().detach()))
        print("step_tail=%-5s  loss %.4e -> %.4e after %d steps" % (tail, out[tail][0], out[tail][1], steps))
    return out


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
