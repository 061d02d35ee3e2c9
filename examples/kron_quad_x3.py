"""The QUAD Kronecker update with its products on the bf16 matrix cores at fp32 grade: products="bf16x3".

First the two functions on one 1024 x 768 layer: the same gradients through the fp32 route and through the bf16 x 3 route
(include/psgd_kron_quad_x3_hip.h), the states compared after every step -- the state is route-independent, so the last steps
switch routes in mid-run.  Then class Kron with quad_products="bf16x3": the wide layer is routed to the new core, the small one
(short side below quad_products_min_dim) stays on the fp32 calls.

    python examples/kron_quad_x3.py [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


def main(steps=20):
    assert torch.cuda.is_available(), "this example runs on the HIP device"
    dev = torch.device("cuda:0")
    M, N = 1024, 768
    gen = torch.Generator(device=dev).manual_seed(0)
    scale = torch.logspace(-1, 1, N, device=dev)
    state = {r: psgd.kron_quad_initial_state(M, N, device=dev) for r in ("fp32", "bf16x3")}
    for k in range(steps):
        G = torch.randn(M, N, device=dev, generator=gen) * scale
        for r, (Ql, Qr, L) in state.items():
            route = r if k < steps - 2 else "fp32" if r == "bf16x3" else "bf16x3"     # the last two steps: routes swapped
            psgd.update_precond_kron_quad_(Ql, Qr, L, G, 0.1, products=route)
    G = torch.randn(M, N, device=dev, generator=gen) * scale
    a = psgd.precond_grad_kron_quad(*state["fp32"][:2], G)
    b = psgd.precond_grad_kron_quad(*state["bf16x3"][:2], G, products="bf16x3")
    rel = lambda x, y: float((x - y).norm() / y.norm())
    print("after %d steps: Ql differs by %.2e, Qr by %.2e, the preconditioned gradient by %.2e (relative, between the routes)"
          % (steps, rel(state["bf16x3"][0], state["fp32"][0]), rel(state["bf16x3"][1], state["fp32"][1]), rel(b, a)))

    cpu_gen = torch.Generator().manual_seed(1)
    params = [(torch.randn(s, generator=cpu_gen) * 0.1).to(dev).requires_grad_() for s in ((512, 640), (32, 48))]
    targets = [torch.randn(p.shape, generator=cpu_gen).to(dev) for p in params]
    closure = lambda: sum(((p - t) ** 2).mean() for p, t in zip(params, targets))
    opt = psgd.Kron(params, "dense", 1.0, 0.01, 0.1, 1.0, preconditioner_fit="whitening", probe_seed=2,
                    generator=torch.Generator().manual_seed(1), preconditioner_update="quad", quad_products="bf16x3", quad_products_min_dim=256)
    first = float(closure().detach())
    for _ in range(steps):
        opt.step(closure)
    print("class Kron: loss %.4e -> %.4e; quad layers %s, on the bf16 x 3 core %s; 'quad_products' in the state dict: %r"
          % (first, float(closure().detach()), opt.quad_layers, opt.quad_x3_layers, opt.state_dict().get("quad_products")))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
