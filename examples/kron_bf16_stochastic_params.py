"""class Kron on bfloat16 parameters without a float32 master copy: round to nearest stalls, param_rounding="stochastic" goes on.

One 64 x 64 weight matrix W in bfloat16, loss = |W - T|^2 / 2 with a target T near 1.  The entries of W are near 1, where the
bfloat16 spacing is 2^-7, and lr_params is small: once |lr * preconditioned gradient| falls below half a spacing, round to nearest
returns every weight unchanged and the loss stops where it is -- nothing is non-finite, nothing warns.  With
param_rounding="stochastic" each update is formed once in float32 and rounded up or down with the probability that makes the
stored value right in expectation, so the weights keep drifting towards T and the loss keeps falling (down to the noise floor of
the format).

    python examples/kron_bf16_stochastic_params.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


def run(param_rounding, steps, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    target = 1.0 + 0.05 * torch.randn(64, 64, device=dev, generator=gen)
    W = torch.ones(64, 64, device=dev, dtype=torch.bfloat16, requires_grad=True)
    opt = psgd.Kron([W], "dense", lr_params=2e-3, lr_preconditioner=0.05, step_tail="fused",
                    generator=torch.Generator(device=dev).manual_seed(1), param_rounding=param_rounding, param_rounding_seed=2)

    def closure():
        return 0.5 * torch.sum((W.float() - target) ** 2)
    first = float(closure().detach())
    moved = 0
    for k in range(steps):
        before = W.detach().clone()
        opt.step(closure)
        moved += int((W.detach() != before).sum())
    return first, float(closure().detach()), moved


def main(steps=300):
    dev = torch.device("cuda:0")
    out = {}
    for rounding in ("nearest", "stochastic"):
        first, last, moved = out[rounding] = run(rounding, steps, dev)
        print("param_rounding=%-10s loss %.4e -> %.4e after %d steps; weight changes written: %d" % (rounding, first, last, steps, moved))
    return out


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 300)
