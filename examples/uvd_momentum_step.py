#!/usr/bin/env python
"""class UVd with momentum and decoupled weight decay on the fused step tail.

A stiff least-squares problem over several parameter tensors of different shapes.  The optimizer keeps ONE flat fp32 momentum
buffer; with step_tail="fused" the gradients are blended into it by the launch that used to pack them, and the decay is one more
term of the single update launch.  Half way through the run the optimizer is saved and a new one resumes from the file's content.

    python examples/uvd_momentum_step.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


def main(steps=60, verbose=True):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    psgd.manual_seed(0)
    shapes = [(64, 32), (32,), (32, 16), (16,), (16, 1)]
    params = [(torch.randn(s, device=dev) * 0.5).requires_grad_(True) for s in shapes]
    stiff = [torch.logspace(-2, 2, p.numel(), device=dev).view(p.shape) for p in params]           # condition number 1e4

    def closure():
        return sum(0.5 * torch.sum(a * p * p) for a, p in zip(stiff, params))

    def make():
        return psgd.UVd(params, rank_of_modification=10, lr_params=0.1, lr_preconditioner=0.1, grad_clip_max_norm=10.0,
                        step_tail="fused", momentum=0.9, weight_decay=1e-4)
    opt = make()
    first = float(closure())
    for k in range(steps // 2):
        loss = opt.step(closure)
    saved = {"uvd": opt.state_dict(), "cuda_rng": torch.cuda.get_rng_state()}
    assert saved["uvd"]["momentum_step"] == steps // 2 and saved["uvd"]["momentum_buffer"].dtype == torch.float32
    opt = make()                                                   # a new optimizer: the load replaces its state and its buffer
    opt.load_state_dict(saved["uvd"])
    torch.cuda.set_rng_state(saved["cuda_rng"])
    for k in range(steps // 2, steps):
        loss = opt.step(closure)
        if verbose and k % 10 == 9:
            print("step %3d  loss %.4e" % (k + 1, float(loss)))
    opt.momentum.assign(0.5)                                       # hyper-parameters are mutable between steps
    opt.step(closure)
    last = float(closure())
    if verbose:
        print("loss %.4e -> %.4e" % (first, last))
    return first, last


if __name__ == "__main__":
    f, l = main()
    assert l < 1e-2 * f, (f, l)
