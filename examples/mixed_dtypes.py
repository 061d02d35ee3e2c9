"""mixed_dtypes=True: a small MLP with bfloat16 WEIGHTS and float32 biases and gains under ONE optimizer, once class Kron
(any_rank=True) and once class UVd, with decoupled weight decay on the weights only through param_groups.

    weights W1, W2 (bfloat16)       the implicit last group: it follows opt.weight_decay
    gain, b1, b2 (float32)          {"params": [...], "weight_decay": 0.0}

Each tensor is updated as in a one-dtype optimizer of its own dtype; on the fused tail every typed launch of the step tail runs once
for the bfloat16 tensors and once for the float32 ones.

    python examples/mixed_dtypes.py [fused|torch]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

IN, HIDDEN, CLASSES = 16, 32, 4


def main(kind="Kron", steps=60, step_tail="fused", seed=0, quiet=False):
    """Returns (losses before each step, opt)."""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(seed)
    weight = lambda *shape: (torch.randn(shape, generator=gen) * shape[0] ** -0.5).to(dev).to(torch.bfloat16).requires_grad_()
    W1, W2 = weight(IN, HIDDEN), weight(HIDDEN, CLASSES)
    gain = torch.ones(HIDDEN, device=dev, requires_grad=True)
    b1, b2 = (torch.zeros(n, device=dev, requires_grad=True) for n in (HIDDEN, CLASSES))
    x = torch.randn(256, IN, generator=gen).to(dev)
    labels = (x[:, :CLASSES].argmax(1)).to(dev)
    torch.manual_seed(seed)                                            # class UVd draws its probe vectors from the global generator

    def closure():
        h = torch.tanh((x @ W1.float()) * gain + b1)
        return torch.nn.functional.cross_entropy(h @ W2.float() + b2, labels)

    params = [W1, gain, b1, W2, b2]
    shared = dict(lr_params=0.05, lr_preconditioner=0.1, grad_clip_max_norm=10.0, step_tail=step_tail, weight_decay=0.01,
                  generator=torch.Generator().manual_seed(seed), mixed_dtypes=True,
                  param_groups=[{"params": [gain, b1, b2], "weight_decay": 0.0}])
    if kind == "Kron":
        opt = psgd.Kron(params, any_rank=True, **shared)
    else:
        opt = psgd.UVd(params, rank_of_modification=10, **shared)
    losses = []
    for k in range(steps):
        losses.append(float(opt.step(closure).detach()))
        if not quiet and k % 10 == 0:
            print("%s step %3d  loss %.4f" % (kind, k, losses[-1]))
    if not quiet:
        print("%s: loss %.4f -> %.4f; dtypes %s; groups %s"
              % (kind, losses[0], losses[-1], [str(p.dtype)[6:] for p in params], opt.param_groups))
    return losses, opt


if __name__ == "__main__":
    tail = sys.argv[1] if len(sys.argv) > 1 else "fused"
    main("Kron", step_tail=tail)
    main("UVd", step_tail=tail)
