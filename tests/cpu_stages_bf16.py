"""CPU stage backend for tests/test_sharded_bf16_cpu.py.  TEST INFRASTRUCTURE ONLY.

Implements the stage interface of psgd_tf_amd.sharded.HipStagesBf16 with NumPy: U, V, d are bfloat16 CPU tensors, the stages
widen them to fp64, compute there and narrow what they write with round to nearest even (the rounding mode, seed and row0 they
are handed are recorded, not used: there is no stochastic stream to emulate at fp64).  What is under test is the choreography
of the bf16 route: which send region is exchanged after which stage, and that every rank ends up with the same reduced values.
The r x r algebra and the row-local update are those of tests/cpu_stages.NumpyStages, called on the scaled Gram.
"""
import numpy as np
import torch

from tests.cpu_stages import NumpyStages


def _w(t):
    return t.to(torch.float64).numpy().copy()


def _narrow_into(t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(torch.bfloat16).reshape(t.shape))


class NumpyBf16Stages:
    def __init__(self, r):
        self.r = r
        nc = 2 * r + 2
        self._s = {1: torch.zeros(r, dtype=torch.float64), 2: torch.zeros(r, dtype=torch.float64),
                   10: torch.zeros(2, dtype=torch.float64), 11: torch.zeros(nc * nc, dtype=torch.float64),
                   12: torch.zeros(1, dtype=torch.float64)}
        self._math = NumpyStages(r)
        self.log = []            # the stages exchanged, in order
        self.narrow_args = []    # (stage name, mode, seed, row0) of every narrowing stage

    # ---- exchange half
    def send(self, stage):
        return self._s[stage]

    def gather_buf(self, stage, world):
        return torch.empty(world * self._s[stage].numel(), dtype=torch.float64)

    def fold(self, stage, gathered, world):
        self.log.append(stage)
        g = gathered.view(world, -1)
        acc = g[0].clone()
        for k in range(1, world):                      # rank order
            acc = torch.maximum(acc, g[k]) if stage in (10, 12) else acc + g[k]
        self._s[stage][:] = acc

    # ---- update
    def balance_max(self, U, V):
        self._s[10][:] = torch.tensor([np.max(np.abs(_w(U))), np.max(np.abs(_w(V)))], dtype=torch.float64)

    def update_gram(self, U, V, d, v, h):
        Un, Vn, dn, vn, hn = map(_w, (U, V, d, v, h))
        W = np.concatenate([Un, Vn, dn * hn, vn / dn], axis=1)
        self._s[11][:] = torch.from_numpy((W.T @ W).ravel())

    def update_rewrite(self, U, V, d, v, h, step, tiny, balance, update_U, mode, seed, row0):
        self.narrow_args.append(("rewrite", mode, seed, row0))
        r = self.r
        Un, Vn, dn, vn, hn = map(_w, (U, V, d, v, h))
        su = sv = 1.0
        if balance:
            m = self._s[10].numpy()
            rho = np.sqrt(m[0] / m[1])
            su, sv = 1.0 / rho, rho
        Un *= su
        Vn *= sv
        D = np.concatenate([np.full(r, su), np.full(r, sv), np.ones(2)])
        G = self._s[11].numpy().reshape(2 * r + 2, 2 * r + 2)
        self._math._sums[11][:] = torch.from_numpy((D[:, None] * G * D[None, :]).ravel())
        self._math.update_sweep2(Un, Vn, dn, vn, hn, step, tiny, update_U)      # updates Un or Vn in place
        self._s[12][:] = float(np.float32(np.max(np.abs(self._math.nabla))))
        if update_U or balance:
            _narrow_into(U, Un)
        if (not update_U) or balance:
            _narrow_into(V, Vn)

    def update_d(self, d, step, tiny, mode, seed, row0):
        self.narrow_args.append(("d", mode, seed, row0))
        dn = _w(d)
        mu = step / (float(self._s[12][0]) + tiny)
        _narrow_into(d, dn - mu * dn * self._math.nabla)

    # ---- apply
    def apply_sweep1(self, V, d, g):
        self._s[1][:] = torch.from_numpy((_w(V).T @ (_w(d) * _w(g))).ravel())

    def apply_sweep1_d(self, V, d, g, step, tiny, mode, seed, row0):
        self.update_d(d, step, tiny, mode, seed, row0)
        self.apply_sweep1(V, d, g)

    def apply_sweep2(self, U, d, g, out=None):
        Un = _w(U)
        self._g1 = _w(d) * _w(g) + Un @ self._s[1].numpy().reshape(-1, 1)
        self._s[2][:] = torch.from_numpy((Un.T @ self._g1).ravel())

    def apply_sweep3(self, V, d):
        return torch.from_numpy(_w(d) * (self._g1 + _w(V) @ self._s[2].numpy().reshape(-1, 1)))
