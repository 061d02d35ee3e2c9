#!/usr/bin/env python
"""class UVd on float16 parameters with a dynamic loss scale and a step that is skipped on overflow.

The closure returns the plain loss; the optimizer differentiates loss * S, takes 1 / S back where it packs the gradients and the
Hessian-vector products (with step_tail="fused" the packs also check what they write), and skips a step in which any of them is
not finite: nothing of the optimizer or the parameters changes, S halves, and the run goes on.  Step 12 gets an overflow injected.

    python examples/uvd_guarded_fp16_step.py
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


def main(steps=24, verbose=True):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    psgd.manual_seed(0)
    shapes = [(64, 32), (32,), (32, 16), (16,)]
    params = [(torch.randn(s, device=dev) * 0.5).half().requires_grad_(True) for s in shapes]
    stiff = [torch.logspace(-1, 1, p.numel(), device=dev).view(p.shape) for p in params]
    inject = {"factor": 1.0}

    def closure():                                   # float16 parameters, the loss accumulated in float32
        return inject["factor"] * sum(0.5 * torch.sum(a * p.float() * p.float()) for a, p in zip(stiff, params))
    opt = psgd.UVd(params, rank_of_modification=10, lr_params=0.05, lr_preconditioner=0.1, grad_clip_max_norm=10.0,
                   step_tail="fused", momentum=0.9, nonfinite="skip", loss_scale="dynamic", loss_scale_growth_interval=8)
    first = float(closure().detach())
    for k in range(steps):
        inject["factor"] = math.inf if k == 12 else 1.0
        loss = opt.step(closure)
        if verbose:
            print("step %2d  loss %.4e  loss_scale 2^%d  %s  skipped_steps %d"
                  % (k, float(loss.detach()), int(math.log2(float(opt.loss_scale))), "SKIPPED" if opt.last_step_skipped else "taken  ",
                     opt.skipped_steps))
    inject["factor"] = 1.0
    last = float(closure().detach())
    assert all(bool(torch.isfinite(p).all()) for p in params)
    if verbose:
        print("loss %.4e -> %.4e, %d of %d steps skipped" % (first, last, opt.skipped_steps, steps))
    return first, last, opt.skipped_steps


if __name__ == "__main__":
    f, l, skipped = main()
    assert skipped >= 1 and math.isfinite(l) and l < f, (f, l, skipped)
