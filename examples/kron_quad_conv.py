"""class Kron with preconditioner_update="quad", any_rank=True, quad_tensor=True: a conv net with one factor per kernel mode.

Two 3 x 3 convolutions and a linear head learn the outputs of a hidden net of the same form.  With quad_tensor=True each conv
kernel [Cout, Cin, 3, 3] is the tensor [Cout, Cin, 9] with three symmetric factors -- output channels, input channels, filter
taps -- updated by update_precond_kron_quad_nd_ and applied by precond_grad_kron_quad_nd (include/psgd_kron_quad_nd_hip.h);
without it the kernel is folded to [Cout, 9 Cin] and the right factor is (9 Cin)^2.  The head and the biases keep their matrix and
vector layers.  The step is bounded with grad_clip_max_norm, as in examples/kron_quad_class.py.

    python examples/kron_quad_conv.py [steps]
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

CH, BATCH, SIDE, OUT = (3, 16, 32), 64, 12, 10


def net(params, x):
    w1, b1, w2, b2, head = params
    x = torch.tanh(F.conv2d(x, w1, b1, padding=1))
    x = torch.tanh(F.conv2d(x, w2, b2, padding=1))
    return x.mean((2, 3)) @ head


def model(dev):
    gen = torch.Generator().manual_seed(0)
    shapes = [(CH[1], CH[0], 3, 3), (CH[1],), (CH[2], CH[1], 3, 3), (CH[2],), (CH[2], OUT)]
    make = lambda scale: [(torch.randn(s, generator=gen) * scale).to(dev) for s in shapes]
    hidden, params = make(0.3), [p.requires_grad_() for p in make(0.1)]
    draw = torch.Generator(device=dev).manual_seed(1)

    def closure():
        x = torch.randn(BATCH, CH[0], SIDE, SIDE, device=dev, generator=draw)
        return ((net(params, x) - net(hidden, x)) ** 2).mean()
    return params, closure


def main(steps=200):
    assert torch.cuda.is_available(), "this example runs on the HIP device"
    dev = torch.device("cuda:0")
    params, closure = model(dev)
    opt = psgd.Kron(params, "dense", 1.0, 0.01, 0.1, 1.0, preconditioner_fit="whitening", probe_seed=2,
                    generator=torch.Generator().manual_seed(1), preconditioner_update="quad", any_rank=True, quad_tensor=True)
    first = sum(float(closure().detach()) for _ in range(8)) / 8
    for _ in range(steps):
        opt.step(closure)
    last = sum(float(closure().detach()) for _ in range(8)) / 8
    print("loss %.4e -> %.4e after %d steps; quad layers %s, of them tensor layers %s"
          % (first, last, steps, opt.quad_layers, opt.quad_tensor_layers))
    for i in opt.quad_tensor_layers:
        Qs = opt.factors[i]
        print("  parameter %d %s: factors %s, L = %s, symmetric: %s"
              % (i, tuple(params[i].shape), [tuple(Q.shape) for Q in Qs], ["%.3g" % v for v in opt.quad_L[i].tolist()],
                 all(bool(torch.equal(Q, Q.T)) for Q in Qs)))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
