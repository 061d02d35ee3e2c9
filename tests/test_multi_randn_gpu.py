"""psgd_multi_randn_f32 through its wrapper (kron_optimizer.multi_randn) on the GPU: against the float64 restatement counter_randn on
lists chosen for odd global indices, unaligned starts, the chunk of 4096 elements and the grid cap of 2048 workgroups; bit-level
invariance under the cut of the list, the call and the stream; the moments of the fixed stream."""
import numpy as np
import pytest
import torch

from tests.multi_randn_cases import MOMENT_N, MOMENT_SEED, moment_figures, reference as _reference

pytestmark = pytest.mark.gpu

CHUNK, MAX_GRID = 4096, 2048
COUNTS = [1, 2, 3, 63, 64, 65, 255, 257, 1023, 4099]               # odd counts: later segments start on odd global indices
GRID_STRIDE = [6] * 2100 + [5000]                                  # 2102 chunks > 2048 workgroups: the second trip of the loop
SENTINEL = 0x5EA7BEEF                                              # the int32 pattern around every tensor
# The largest |kernel - counter_randn| measured over the 2^20 draws of the fixed stream (scale 1) on an MI355X, and the bar of
# these tests: four times that, the margin for math-library differences between ROCm builds (profiles/kron_whitening.txt).
# The bar is taken against the float64 restatement, never against an earlier output of the kernel.
PROBE_ERR_MEASURED = 9.5367e-07                                    # two float32 ulps at |z| = 4.03
BAR = 4.0 * PROBE_ERR_MEASURED


@pytest.fixture(scope="module")
def ko():
    from psgd_tf_amd import _lib, kron_optimizer
    assert _lib.UVD_TAIL_CHUNK == CHUNK and _lib.UVD_TAIL_MAX_GRID == MAX_GRID
    assert sum(-(-n // CHUNK) for n in GRID_STRIDE) > MAX_GRID
    return kron_optimizer


@pytest.fixture(scope="module")
def psgd():
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


def _carve(sizes, offsets):
    """tensors of these element counts inside ONE int32-sentinel buffer, tensor i starting offsets[i] floats past a 16-byte
    boundary, at least one sentinel element between neighbours and on both ends; the tensors themselves are poisoned with NaN.
    Returns (buffer, tensors, mask of the buffer's elements that belong to no tensor)."""
    starts, pos = [], 0
    for n, o in zip(sizes, offsets):
        pos = (pos + 1 + 3) // 4 * 4 + o
        starts.append(pos)
        pos += n
    buf = torch.full((pos + 5,), SENTINEL, dtype=torch.int32, device=_dev()).view(torch.float32)
    assert buf.data_ptr() % 16 == 0
    outside = torch.ones(buf.numel(), dtype=torch.bool, device=_dev())
    ts = []
    for s, n in zip(starts, sizes):
        t = buf[s:s + n]
        assert t.data_ptr() % 16 == (4 * s) % 16
        t.fill_(float("nan"))
        outside[s:s + n] = False
        ts.append(t)
    return buf, ts, outside


def _sentinels_kept(buf, outside):
    return bool((buf.view(torch.int32)[outside] == SENTINEL).all())


def _tolerance(want, scale):
    """|kernel - restatement| at scale s: s times the bar of scale 1, plus the two roundings the scaled values differ by (the
    kernel rounds s * z_kernel, the restatement s * z_restated: half an ulp of the result each)"""
    return abs(scale) * BAR + 2.0 ** -23 * np.abs(want.astype(np.float64))


def _check(psgd, ts, seed, index0, scale):
    n = sum(int(t.numel()) for t in ts)
    got = torch.cat([t.reshape(-1) for t in ts]).cpu().numpy()
    assert np.all(np.isfinite(got)), "an element was not written (NaN poison) or is not finite"
    want = np.float32(scale) * _reference(psgd, seed, index0, n)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = _tolerance(want, scale)
    print("index0 %d, scale %g: max |kernel - restatement| %.3e (bar %.3e)" % (index0, scale, err.max(), abs(scale) * BAR))
    assert np.all(err <= tol), (float(err.max()), int(np.argmax(err - tol)))
    return got


# ------------------------------------------------------------------------------------------------ the measured distance, the bar
def test_distance_to_the_restatement_on_the_fixed_stream(ko, psgd):
    """the figure behind BAR, measured again: 2^20 draws in one tensor"""
    out = torch.full((MOMENT_N,), float("nan"), device=_dev())
    ko.multi_randn([out], MOMENT_SEED)
    got = out.cpu().numpy().astype(np.float64)
    want = _reference(psgd, MOMENT_SEED, 0, MOMENT_N).astype(np.float64)
    err = np.abs(got - want)
    i = int(np.argmax(err))
    print("max |kernel - restatement| over 2^20 draws: %.4e at element %d (z = %.6f); mean %.3e" % (err[i], i, want[i], err.mean()))
    assert err[i] <= 8e-6                              # beyond about 16 ulps at |z| = 6.67 the kernel has a bug, whatever the bar says
    assert err[i] <= BAR


# --------------------------------------------------------------------------------------------------- against counter_randn
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -12, 3.0])
@pytest.mark.parametrize("index0", [0, 1, 2 ** 33 + 1])
def test_list_against_the_restatement(ko, psgd, index0, scale):
    """tensors at byte offsets 0, 4, 8 and 12 from a 16-byte boundary, every element overwritten, every sentinel kept"""
    seed = psgd.uvd_step_rounding_seed(77, 5)
    offsets = [(i + 1) % 4 for i in range(len(COUNTS))]               # 4, 8, 12, 0, ... bytes
    buf, ts, outside = _carve(COUNTS, offsets)
    assert ko.multi_randn(ts, seed, index0, scale) is not None
    _check(psgd, ts, seed, index0, scale)
    assert _sentinels_kept(buf, outside), "an element outside the tensors was written"


def test_grid_stride_list_against_the_restatement(ko, psgd):
    seed = psgd.uvd_step_rounding_seed(78, 0)
    buf, ts, outside = _carve(GRID_STRIDE, [(2 * i + 1) % 4 for i in range(len(GRID_STRIDE))])
    ko.multi_randn(ts, seed, 3)
    _check(psgd, ts, seed, 3, 1.0)
    assert _sentinels_kept(buf, outside)


def test_empty_tensors_and_argument_errors(ko):
    ts = [torch.full((5,), float("nan"), device=_dev()), torch.zeros(0, device=_dev()), torch.full((2, 3), float("nan"), device=_dev())]
    ko.multi_randn(ts, 1)
    assert all(bool(torch.isfinite(t).all()) for t in ts)
    assert ko.multi_randn([torch.zeros(0, device=_dev())], 1) is not None          # nothing to write: no launch
    with pytest.raises(ValueError, match="index0"):
        ko.multi_randn(ts, 1, -1)
    with pytest.raises(ValueError, match="scale"):
        ko.multi_randn(ts, 1, 0, float("inf"))
    with pytest.raises(TypeError, match="float32"):
        ko.multi_randn([torch.zeros(4, device=_dev(), dtype=torch.bfloat16)], 1)
    with pytest.raises(ValueError, match="not contiguous"):
        ko.multi_randn([torch.zeros(4, 6, device=_dev()).t()], 1)
    with pytest.raises(Exception, match="HIP device"):
        ko.multi_randn([torch.zeros(4)], 1)


# ------------------------------------------------------------------------------------------------------ bit-level invariances
def _bits(ts):
    return torch.cat([t.reshape(-1) for t in ts]).view(torch.int32).clone()


@pytest.mark.parametrize("index0", [0, 1, 2 ** 33 + 1])
def test_the_cut_of_the_list_the_call_and_the_stream_do_not_move_a_bit(ko, psgd, index0):
    seed = psgd.uvd_step_rounding_seed(79, 2)
    n = sum(COUNTS)
    one = torch.full((n,), float("nan"), device=_dev())
    ko.multi_randn([one], seed, index0)
    whole = _bits([one])
    # the same n elements cut into the list, at other alignments
    _, ts, _ = _carve(COUNTS, [(i + 1) % 4 for i in range(len(COUNTS))])
    ko.multi_randn(ts, seed, index0)
    assert torch.equal(_bits(ts), whole), "the cut of the list moved a bit"
    # another cut, other alignments, one chunk boundary inside a tensor
    cut2 = [CHUNK + 1, n - CHUNK - 1 - 7, 7]
    _, ts2, _ = _carve(cut2, [3, 2, 1])
    ko.multi_randn(ts2, seed, index0)
    assert torch.equal(_bits(ts2), whole), "a second cut moved a bit"
    # a tail of the stream alone: the draws are keyed by the global index
    tail = torch.full((n - 65,), float("nan"), device=_dev())
    ko.multi_randn([tail], seed, index0 + 65)
    assert torch.equal(_bits([tail]), whole[65:])
    # a second call
    for t in ts:
        t.fill_(float("nan"))
    ko.multi_randn(ts, seed, index0)
    assert torch.equal(_bits(ts), whole), "a second call moved a bit"
    # a non-default stream, with a plan of its own (calls that share a plan run on one stream)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        _, ts3, _ = _carve(COUNTS, [(i + 2) % 4 for i in range(len(COUNTS))])
        ko.multi_randn(ts3, seed, index0, plan=ko.MultiTailPlan(COUNTS, _dev()))
        got = _bits(ts3)
    side.synchronize()
    assert torch.equal(got, whole), "a non-default stream moved a bit"
    # (MultiTailPlan has one chunking, PSGD_UVD_TAIL_CHUNK: there is no second chunking to compare with)


# ------------------------------------------------------------------------------------------------------------------- moments
def test_moments_of_the_fixed_stream_on_the_kernels_output(ko):
    out = torch.full((MOMENT_N,), float("nan"), device=_dev())
    ko.multi_randn([out], MOMENT_SEED)
    z = out.cpu().numpy()
    assert np.all(np.isfinite(z))
    for name, (value, bound) in moment_figures(z).items():
        print("%-17s %.3e (bound %.3e)" % (name, value, bound))
        assert value <= bound, name
