"""class Kron on `list(model.parameters())` of an ordinary torch.nn.Module: a conv layer, a LayerNorm and a linear layer, with their
biases.  Kron(any_rank=True) takes the rank-4 conv kernel as the matrix layer [out, in * kh * kw], every bias and LayerNorm vector
as a vector layer (the reference's [1, n] layer in the ("dense", "scale") format: a diagonal preconditioner with one scalar of
balance), and updates all vectors of a step in one launch and applies them in one launch.

Synthetic data: random images and random targets, a regression loss.  The convolution is written as a product with the unfolded
patches (torch.nn.functional.unfold) so that its Hessian-vector products are plain matrix products.

    python examples/kron_module_parameters.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 8, 3)                   # weight [8, 3, 3, 3], bias [8]
        self.norm = torch.nn.LayerNorm(8 * 36)                  # weight [288], bias [288]
        self.head = torch.nn.Linear(8 * 36, 10)                 # weight [10, 288], bias [10]

    def forward(self, x):
        cols = torch.nn.functional.unfold(x, 3)                                                    # [B, 27, 36] for 8 x 8 images
        h = torch.tanh(self.conv.weight.reshape(8, 27) @ cols + self.conv.bias[None, :, None])     # the convolution
        return self.head(self.norm(h.flatten(1)))


def main(steps=100):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Net().to(dev)
    x, y = torch.randn(64, 3, 8, 8, device=dev), torch.randn(64, 10, device=dev)
    params = list(model.parameters())
    opt = psgd.Kron(params, "dense", lr_params=0.05, lr_preconditioner=0.1, grad_clip_max_norm=10.0, step_tail="fused",
                    generator=torch.Generator(device=dev).manual_seed(0), any_rank=True)
    for (name, p), (kind, shape, fmt), pair in zip(model.named_parameters(), psgd.kron_layers([p.shape for p in params], "dense", True),
                                                   opt.factors):
        print("%-12s %-16s -> %-6s layer %-10s %-18s factors %s, %s"
              % (name, tuple(p.shape), kind, shape, fmt, tuple(pair[0].shape), tuple(pair[1].shape)))

    def closure():
        return torch.nn.functional.mse_loss(model(x), y)
    first = float(closure().detach())
    for _ in range(steps):
        opt.step(closure)
    last = float(closure().detach())
    print("loss %.4e -> %.4e after %d steps" % (first, last, steps))
    return first, last


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 100)
