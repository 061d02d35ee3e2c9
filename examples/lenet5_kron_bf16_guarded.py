"""class Kron on bfloat16 parameters with the guarded step and a dynamic loss scale, on the LeNet5 weight shapes of the reference's
mnist_with_lenet5.py (:12-16): the parameters are bfloat16, the Kronecker factors and the momentum buffers stay float32, and only
the parameter update is rounded to bfloat16.

Synthetic data: there is no MNIST here.  The loss is the quadratic of examples/lenet5_kron_class.py on the widened parameters, so
autograd hands back bfloat16 gradients.  One step sees an Inf gradient (a multiplier in the loss is set to Inf for that step, as an
overflow in the backward pass would do it): the step is skipped, nothing is damaged, the loss scale halves, and the run goes on.

    python examples/lenet5_kron_bf16_guarded.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

SHAPES = [(26, 6), (151, 16), (257, 120), (121, 84), (85, 10)]          # W1 .. W5 of mnist_with_lenet5.py:12-16


def main(steps=12, bad_step=5):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    Hl = [torch.diag(torch.exp(torch.empty(m, device=dev).uniform_(-1.5, 1.5, generator=g))) for m, n in SHAPES]
    Hr = [torch.diag(torch.exp(torch.empty(n, device=dev).uniform_(-1.5, 1.5, generator=g))) for m, n in SHAPES]
    Ws = [torch.randn(m, n, device=dev, generator=g).bfloat16().requires_grad_(True) for m, n in SHAPES]
    clip = 0.1 * sum(W.numel() for W in Ws) ** 0.5                                                  # :63
    opt = psgd.Kron(Ws, "dense", lr_params=0.1, lr_preconditioner=0.1, grad_clip_max_norm=clip, step_tail="fused", generator=g,
                    momentum=0.9, weight_decay=1e-4, nonfinite="skip", loss_scale="dynamic", loss_scale_growth_interval=4)
    overflow = torch.ones((), device=dev)

    def closure():
        return sum(0.5 * torch.sum(W.float() * (hl @ W.float() @ hr)) for W, hl, hr in zip(Ws, Hl, Hr)) * overflow
    first = float(closure().detach())
    for k in range(1, steps + 1):
        overflow.fill_(float("inf") if k == bad_step else 1.0)
        opt.step(closure)
        print("step %2d  %s  loss_scale 2^%d  skipped_steps %d"
              % (k, "SKIPPED" if opt.last_step_skipped else "taken  ", round(torch.log2(torch.tensor(float(opt.loss_scale))).item()),
                 opt.skipped_steps))
    overflow.fill_(1.0)
    last = float(closure().detach())
    assert opt.skipped_steps == 1 and last < first
    assert all(W.dtype == torch.bfloat16 and bool(torch.isfinite(W).all()) for W in Ws)
    assert all(q.dtype == torch.float32 for pair in opt.factors for q in pair)
    print("loss %.4e -> %.4e after %d steps on bfloat16 parameters, skipped_steps = %d" % (first, last, steps, opt.skipped_steps))
    return first, last, opt.skipped_steps


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 12)
