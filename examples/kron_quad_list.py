"""class Kron with the QUAD update on a dozen small dense layers, with quad_route="layer" (10 launches per layer and step) and
quad_route="list" (10 launches per step for all of them: kron_quad_list.py, psgd_kron_qlist.hip).  Both routes compute the same
bits, so the two runs print the same losses and end on identical parameters.

Synthetic data: the loss is the separable quadratic of examples/kron_quad_class.py, sum_i |W_i - T_i|^2.

    python examples/kron_quad_list.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

SHAPES = [(26, 6), (151, 16), (257, 120), (121, 84), (85, 10), (64, 64)] * 2


def run(route, steps, dev):
    gen = torch.Generator().manual_seed(0)
    params = [torch.randn(s, generator=gen).to(dev).requires_grad_() for s in SHAPES]
    targets = [torch.randn(s, generator=gen).to(dev) for s in SHAPES]
    closure = lambda: sum(((x - t) ** 2).sum() for x, t in zip(params, targets))
    opt = psgd.Kron(params, "dense", 1.0, 0.05, 0.1, preconditioner_fit="whitening", probe_seed=3, preconditioner_update="quad",
                    generator=torch.Generator().manual_seed(1), quad_route=route)
    for step in range(steps):
        loss = opt.step(closure)
        if step % 10 == 0 or step == steps - 1:
            print("%-5s step %3d  loss %.6e" % (route, step, float(loss)))
    return params


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    assert torch.cuda.is_available(), "this example needs the HIP device: there is no CPU fallback"
    dev = torch.device("cuda:0")
    a, b = run("layer", steps, dev), run("list", steps, dev)
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    print("parameters bit-identical between the routes: %s" % same)
    assert same


if __name__ == "__main__":
    main()
