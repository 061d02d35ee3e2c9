"""param_groups= on class UVd: a small MLP on token ids -- an embedding table, two linear layers with biases -- trained with
decoupled weight decay on the WEIGHTS only and a FROZEN embedding, under one preconditioner over all five tensors.

    {"params": biases,      "weight_decay": 0.0}                       no decay; lr_scale defaults to 1.0
    {"params": [embedding], "lr_scale": 0.0, "weight_decay": 0.0}      frozen: its bits do not move
    the two weight matrices: the implicit last group, which follows opt.weight_decay

After half of the steps the embedding is thawed at a tenth of the learning rate through its _Hyper object.

    python examples/param_groups.py [fused|torch]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

VOCAB, DIM, HIDDEN, CLASSES = 50, 16, 32, 4


def main(steps=60, step_tail="fused", seed=0, quiet=False):
    """Returns (losses before each step, the embedding's bits moved while frozen?, opt)."""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(seed)
    make = lambda *shape: (torch.randn(shape, generator=gen) * shape[0] ** -0.5).to(dev).requires_grad_()
    emb, W1, W2 = make(VOCAB, DIM), make(DIM, HIDDEN), make(HIDDEN, CLASSES)
    b1, b2 = (torch.zeros(n, device=dev, requires_grad=True) for n in (HIDDEN, CLASSES))
    tokens = torch.randint(0, VOCAB, (256,), generator=gen).to(dev)
    labels = (tokens % CLASSES).to(dev)
    torch.manual_seed(seed)                                            # the probe vectors of the step come from the global generator

    def closure():
        h = torch.tanh(emb[tokens] @ W1 + b1)
        return torch.nn.functional.cross_entropy(h @ W2 + b2, labels)

    opt = psgd.UVd([emb, W1, b1, W2, b2], rank_of_modification=10, lr_params=0.05, lr_preconditioner=0.1, grad_clip_max_norm=10.0,
                   step_tail=step_tail, weight_decay=0.01, generator=torch.Generator().manual_seed(seed),
                   param_groups=[{"params": [b1, b2], "weight_decay": 0.0},
                                 {"params": [emb], "lr_scale": 0.0, "weight_decay": 0.0}])
    frozen = opt.param_groups[1]
    emb0, losses, moved = emb.detach().clone(), [], False
    for k in range(steps):
        if k == steps // 2:
            moved = not torch.equal(emb.detach(), emb0)
            frozen.lr_scale.assign(0.1)                                # a schedule: takes effect at this step
        losses.append(float(opt.step(closure).detach()))
        if not quiet and k % 10 == 0:
            print("step %3d  loss %.4f" % (k, losses[-1]))
    if not quiet:
        print("groups:", opt.param_groups)
        print("loss %.4f -> %.4f; embedding moved while frozen: %s, after the thaw: %s"
              % (losses[0], losses[-1], moved, not torch.equal(emb.detach(), emb0)))
    return losses, moved, opt


if __name__ == "__main__":
    main(step_tail=sys.argv[1] if len(sys.argv) > 1 else "fused")
