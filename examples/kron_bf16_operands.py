"""class Kron with operands="bfloat16": a two-layer module whose weight matrices run on the bf16-operand Kron kernels while the
biases stay on the fp32 vector kernels.  The factors stay float32; dX, dG and the gradient of an operand layer are rounded to
bfloat16 once per step (one launch for all layers each), and its preconditioned gradient comes back as a bfloat16 tensor that
the fused tail reads as float.  operand_min_dim=8 makes these small layers qualify; the default (768) is where the bf16 route
starts to pay on the MI355X.

    python examples/kron_bf16_operands.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


def main(steps=50):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(24, 40), torch.nn.Tanh(), torch.nn.Linear(40, 8)).to(dev)
    x, y = torch.randn(128, 24, device=dev), torch.randn(128, 8, device=dev)
    params = list(model.parameters())
    opt = psgd.Kron(params, "dense", lr_params=0.05, lr_preconditioner=0.1, grad_clip_max_norm=10.0, step_tail="fused",
                    generator=torch.Generator(device=dev).manual_seed(0), any_rank=True, momentum=0.9,
                    operands="bfloat16", operand_min_dim=8)
    names = [n for n, _ in model.named_parameters()]
    print("operand layers:", [names[i] for i in opt.operand_layers])

    def closure():
        return torch.nn.functional.mse_loss(model(x), y)
    first = float(closure().detach())
    for k in range(steps):
        loss = opt.step(closure)
        if k % 10 == 0:
            print("step %3d loss %.4e" % (k, float(loss.detach())))
    last = float(closure().detach())
    print("loss %.4e -> %.4e after %d steps" % (first, last, steps))
    return first, last


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 50)
