"""class Kron on a stack of conv kernels with one factor per tensor mode, per-layer calls (quad_tensor_route="layer": 13 launches
per layer and step) against the grouped route (quad_tensor_route="list": at most 14 per step for all of them; kron_quad_nd_list.py,
psgd_kron_qtlist.hip).  At these shapes no Gram is split, so both routes compute the same bits; the script checks that and prints
the slice counts a wider kernel would get.

    python examples/kron_quad_conv_list.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402
from psgd_tf_amd import kron_quad_nd_list  # noqa: E402

SHAPES = [(16, 3, 3, 3), (32, 16, 3, 3), (32, 32, 3, 3), (64, 32, 1, 1), (10, 64)]


def run(route, steps, dev):
    gen = torch.Generator().manual_seed(0)
    params = [(0.1 * torch.randn(s, generator=gen)).to(dev).requires_grad_() for s in SHAPES]
    targets = [torch.randn(s, generator=gen).to(dev) for s in SHAPES]
    opt = psgd.Kron(params, "dense", 1.0, 0.01, 0.1, preconditioner_fit="whitening", probe_seed=3, preconditioner_update="quad",
                    generator=torch.Generator().manual_seed(1), any_rank=True, quad_tensor=True, quad_tensor_route=route)
    closure = lambda: sum(((x - t) ** 2).sum() for x, t in zip(params, targets))
    for _ in range(steps):
        loss = opt.step(closure)
    return float(torch.as_tensor(loss).detach()), params, opt


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    loss_list, p_list, opt = run("list", steps, dev)
    loss_layer, p_layer, _ = run("layer", steps, dev)
    print("tensor layers %s, slices %s, groups %s" % (opt.quad_tensor_layers, opt.quad_tensor_plan.slices, opt.quad_tensor_plan.groups))
    print("loss after %d steps: list %.6f, layer %.6f" % (steps, loss_list, loss_layer))
    assert all(torch.equal(a, b) for a, b in zip(p_list, p_layer)), "the two routes must agree bit for bit where nothing is split"
    print("a 512 x 512 x 3 x 3 kernel would be split into", kron_quad_nd_list.plan_layers([(512, 512, 9)])["slices"][0], "slices per side")


if __name__ == "__main__":
    main()
