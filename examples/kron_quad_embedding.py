"""class Kron with preconditioner_update="quad", quad_diagonal=True: an embedding table under the inverse-free whitening update.

A 4096 x 64 embedding feeds one 64 x 16 dense layer; the targets are those of a hidden model of the same form.  The table's long
side cannot hold a dense factor at real vocabulary sizes, so its format is ("scale", "dense"): a vector of 4096 row scales and a
64 x 64 symmetric factor.  With quad_diagonal=True that layer joins the (dense, dense) one in opt.quad_layers and both run
update_precond_kron_quad_ / precond_grad_kron_quad (include/psgd_kron_quad_diag_hip.h); with the default it would keep the
triangular update and its probe.  The step is bounded with grad_clip_max_norm, as in examples/kron_quad_class.py.

    python examples/kron_quad_embedding.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

VOCAB, WIDTH, OUT, BATCH = 4096, 64, 16, 2048


def model(dev):
    gen = torch.Generator().manual_seed(0)
    hidden = [torch.randn(VOCAB, WIDTH, generator=gen).to(dev), (torch.randn(WIDTH, OUT, generator=gen) / WIDTH ** 0.5).to(dev)]
    params = [(torch.randn(VOCAB, WIDTH, generator=gen) * 0.1).to(dev).requires_grad_(),
              (torch.randn(WIDTH, OUT, generator=gen) * 0.1).to(dev).requires_grad_()]
    draw = torch.Generator(device=dev).manual_seed(1)

    def closure():
        tokens = torch.randint(0, VOCAB, (BATCH,), device=dev, generator=draw)
        return ((torch.tanh(params[0][tokens]) @ params[1] - torch.tanh(hidden[0][tokens]) @ hidden[1]) ** 2).mean()
    return params, closure


def main(steps=200):
    assert torch.cuda.is_available(), "this example runs on the HIP device"
    dev = torch.device("cuda:0")
    params, closure = model(dev)
    opt = psgd.Kron(params, [("scale", "dense"), "dense"], 1.0, 0.01, 0.1, 1.0, preconditioner_fit="whitening", probe_seed=2,
                    generator=torch.Generator().manual_seed(1), preconditioner_update="quad", quad_diagonal=True)
    first = sum(float(closure().detach()) for _ in range(8)) / 8
    for _ in range(steps):
        opt.step(closure)
    last = sum(float(closure().detach()) for _ in range(8)) / 8
    print("loss %.4e -> %.4e after %d steps; quad layers %s" % (first, last, steps, opt.quad_layers))
    q, Q = opt.factors[0]
    print("  embedding: row scales in [%.3g, %.3g], L = %s, dense factor symmetric: %s"
          % (float(q.min()), float(q.max()), opt.quad_L[0].tolist(), bool(torch.equal(Q, Q.T))))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
