"""GPU: the nine parameter-update entry points of psgd_param_update.hip stand on ONE kernel template; what must hold between them.

Entry points agree: the same (p, g, v, lr, wd, sumsq) gives the same bits through the flat entry point, the list entry point and the
mixed entry point with an all-fp32 list, and -- bf16, stochastic rounding -- through the three _sr entry points with equal seed,
index0 and flat order.

Shortest table wins: with a vs table whose second segment is 5 elements shorter than its parameter every entry point returns PSGD_OK,
updates exactly the common prefix of that tensor and leaves the parameter's last 5 elements as they were.  Every buffer is a real
tensor of full length and only the table's count is shortened: nothing is read or written outside an allocation on any code path.

The bits themselves are pinned against torch by the tests of the wrappers (test_uvd_tail_gpu.py, test_multi_tail*_gpu.py,
test_param_rounding_gpu.py); here the calls go to the C ABI directly, with tables built by hand."""
import numpy as np
import pytest
import torch

from psgd_tf_amd import _lib
from psgd_tf_amd.preconditioned_stochastic_gradient_descent import _TAIL_DTYPES, uvd_tail_chunks

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
GUARD = 8                    # untouched elements behind every view, compared with the rest
MAX_NORM, TINY = 1.0, 1e-30
SEED, INDEX0 = 0x1234567, 1000


def int_view(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


class Operands:
    """k tensors of one role on the device, tensor j a view that starts offs[j] elements into its own buffer"""

    def __init__(self, values, offs, dtype):
        self.bufs, self.views = [], []
        for x, o in zip(values, offs):
            buf = torch.zeros(o + x.numel() + GUARD, dtype=dtype, device=DEV)
            buf[o:o + x.numel()] = x.to(DEV).to(dtype)
            self.bufs.append(buf)
            self.views.append(buf[o:o + x.numel()])

    def table(self, counts=None, starts=None):
        """the device segment table {pointer, start, count}; the caller keeps it alive until the launch has run"""
        k = len(self.views)
        rows = np.zeros((k, 3), dtype=np.int64)
        rows[:, 0] = [v.data_ptr() for v in self.views]
        rows[:, 1] = 0 if starts is None else starts
        rows[:, 2] = [v.numel() for v in self.views] if counts is None else counts
        return torch.from_numpy(rows).to(DEV)

    def bits(self):
        return [int_view(b).clone() for b in self.bufs]


def flat_starts(sizes):
    return list(np.cumsum([0] + list(sizes[:-1])))


def chunk_table(sizes):
    ch = uvd_tail_chunks(sizes)
    return torch.from_numpy(ch).to(DEV), int(ch.shape[0])


def run(lib, name, p_tab, g, v_tab, k, chunks, nchunks, dtype, lr, sumsq, wd):
    """one call of entry point `name`; g is the flat fp32 vector (flat entry points) or a segment table (list entry points), or None"""
    st = torch.cuda.current_stream(DEV).cuda_stream
    code = _TAIL_DTYPES[dtype]
    gp = None if g is None else g.data_ptr()
    vp = None if v_tab is None else v_tab.data_ptr()
    sp = None if sumsq is None else sumsq.data_ptr()
    head = (p_tab.data_ptr(), gp, vp, k, chunks.data_ptr(), nchunks)
    clip = (lr, sp, MAX_NORM, TINY)
    if name.startswith("psgd_uvd"):
        args = (p_tab.data_ptr(), vp, k, chunks.data_ptr(), nchunks, code, gp) + clip
    elif name.endswith("_f32"):
        args = head + clip
    else:
        args = head + (code,) + clip
    if name not in ("psgd_uvd_param_update_multi", "psgd_multi_param_update_f32"):
        args += (wd,)
    if name.endswith("_sr"):
        args += (SEED, INDEX0)
    return getattr(lib, name)(*args, st)


def values(sizes, seed):
    """p of ordinary size, v small, g such that lr * g is a few ulps of p; zeros of both signs, and gradients whose product with lr
    rounds to -0 in fp16"""
    gen = torch.Generator().manual_seed(seed)
    p = [torch.randn(n, generator=gen) for n in sizes]
    g = [torch.randn(n, generator=gen) for n in sizes]
    v = [torch.randn(n, generator=gen) * 2.0 ** -6 for n in sizes]
    for j, n in enumerate(sizes):
        p[j][::5] = -0.0
        g[j][::3] = -1e-9
        if n > 1:
            p[j][1::7] = 0.0
            v[j][1::4] = -0.0
    return p, g, v


SIZES = (1, 7, 8, 9, 4097)
P_OFFS, G_OFFS, V_OFFS = (1, 3, 1, 3, 1), (3, 1, 3, 1, 3), (1, 1, 3, 3, 1)


@pytest.fixture(scope="module")
def problem():
    return values(SIZES, 11)


def routes(lib, names, dtype, problem, vs, wd, sumsq, mixed_code=None):
    """the parameter buffers' bits after each entry point of `names` ran on its own copy of the problem"""
    pv, gv, vv = problem
    k = len(SIZES)
    chunks, nchunks = chunk_table(SIZES)
    starts = flat_starts(SIZES)
    flat = torch.cat(gv).to(DEV)
    out = {}
    for name in names:
        p = Operands(pv, P_OFFS, dtype)
        v = Operands(vv, V_OFFS, dtype)
        g = Operands(gv, G_OFFS, F32)
        p_tab = p.table(starts=starts)
        v_tab = v.table() if vs else None
        if name.startswith("psgd_uvd"):
            g_arg = flat
        else:
            g_arg = g.table(starts=_lib.DTYPE_F32 if "mixed" in name else None)
        rc = run(lib, name, p_tab, g_arg, v_tab, k, chunks, nchunks, dtype, 0.5 ** 7, sumsq, wd)
        assert rc == _lib.PSGD_OK, (name, rc)
        torch.cuda.synchronize()
        out[name] = p.bits()
        assert any(not torch.equal(a, int_view(b)) for a, b in zip(out[name], Operands(pv, P_OFFS, dtype).bufs)), name
    return out


def assert_same(out):
    names = list(out)
    for name in names[1:]:
        for j, (a, b) in enumerate(zip(out[names[0]], out[name])):
            assert torch.equal(a, b), "%s and %s differ in tensor %d" % (names[0], name, j)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.25])
@pytest.mark.parametrize("vs", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_entry_points_agree(hip_lib, problem, dtype, vs, wd, clip):
    sumsq = torch.tensor([4.0], dtype=torch.float64, device=DEV) if clip else None      # a norm of 2 against MAX_NORM = 1
    names = ["psgd_uvd_param_update_multi_wd", "psgd_multi_param_update_t", "psgd_multi_param_update_mixed"]
    if wd == 0.0:
        names.append("psgd_uvd_param_update_multi")
    if dtype == F32:
        names.append("psgd_multi_param_update_wd_f32")
        if wd == 0.0:
            names.append("psgd_multi_param_update_f32")
    assert_same(routes(hip_lib, names, dtype, problem, vs, wd, sumsq))
    if dtype == BF16:
        assert_same(routes(hip_lib, ["psgd_uvd_param_update_multi_sr", "psgd_multi_param_update_sr",
                                     "psgd_multi_param_update_mixed_sr"], dtype, problem, vs, wd, sumsq))


ENTRY_DTYPES = [("psgd_uvd_param_update_multi", (F32, BF16, F16)), ("psgd_uvd_param_update_multi_wd", (F32, BF16, F16)),
                ("psgd_uvd_param_update_multi_sr", (BF16,)), ("psgd_multi_param_update_f32", (F32,)),
                ("psgd_multi_param_update_wd_f32", (F32,)), ("psgd_multi_param_update_t", (F32, BF16, F16)),
                ("psgd_multi_param_update_mixed", (F32, BF16, F16)), ("psgd_multi_param_update_sr", (BF16,)),
                ("psgd_multi_param_update_mixed_sr", (BF16,))]


@pytest.mark.parametrize("n", [13, 4101])
@pytest.mark.parametrize("name,dtype", [(nm, dt) for nm, dts in ENTRY_DTYPES for dt in dts])
def test_shortest_table_wins(hip_lib, name, dtype, n):
    sizes, short = (9, n, 8), (9, n - 5, 8)
    offs = (1, 3, 0)
    pv, gv, vv = values(sizes, 12)
    starts = flat_starts(sizes)
    flat = torch.cat(gv).to(DEV)
    wd = 0.0 if name in ("psgd_uvd_param_update_multi", "psgd_multi_param_update_f32") else 0.25
    got = {}
    # "cut": the tables of the full tensors, the chunk table of the full sizes, the vs table alone 5 short in its second segment;
    # "well-formed": the same tensors with every table and the chunk table 5 short there
    for leg, p_counts, chunk_sizes in (("cut", sizes, sizes), ("well-formed", short, short)):
        p = Operands(pv, offs, dtype)
        v = Operands(vv, offs, dtype)
        g = Operands(gv, offs, F32)
        chunks, nchunks = chunk_table(chunk_sizes)
        p_tab, v_tab = p.table(counts=p_counts, starts=starts), v.table(counts=short)
        if name.startswith("psgd_uvd"):
            g_arg = flat
        else:
            g_arg = g.table(counts=p_counts, starts=_lib.DTYPE_F32 if "mixed" in name else None)
        rc = run(hip_lib, name, p_tab, g_arg, v_tab, 3, chunks, nchunks, dtype, 0.5 ** 7, None, wd)
        assert rc == _lib.PSGD_OK, (leg, rc)
        torch.cuda.synchronize()
        got[leg] = p.bits()
    before = Operands(pv, offs, dtype).bits()
    for j in range(3):
        assert torch.equal(got["cut"][j], got["well-formed"][j]), "tensor %d" % j
    o = offs[1]
    assert torch.equal(got["cut"][1][o + n - 5:], before[1][o + n - 5:])
    assert not torch.equal(got["cut"][1][o:o + n - 5], before[1][o:o + n - 5])
