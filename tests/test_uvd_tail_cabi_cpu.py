"""The C ABI of the UVd step tail (psgd_uvd_tail.hip): exported with the header's signatures, bound, argument checks that return
before any HIP call, and the host chunk table.  The arithmetic is checked on the GPU in test_uvd_tail_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from psgd_tf_amd import _lib

NAMES = ("psgd_uvd_pack_f32", "psgd_uvd_sumsq_f32", "psgd_uvd_param_update_multi")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_hip.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


def test_exports_are_bound(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.psgd_abi_version() == 7                      # additive: the version did not move


def test_signatures_and_constants_match_the_header():
    text = open(HEADER).read()
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
    for name in NAMES:
        m = re.search(r"(int64_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is kinds[m.group(1)], name
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is ctypes.c_void_p, (name, p)
            else:
                assert t is kinds[p.split()[0]], (name, p)
    consts = dict(re.findall(r"#define\s+(PSGD_(?:DTYPE_\w+|UVD_TAIL_CHUNK|UVD_SUMSQ_WS_BYTES))\s+(\d+)", text))
    assert int(consts["PSGD_UVD_TAIL_CHUNK"]) == _lib.UVD_TAIL_CHUNK
    assert int(consts["PSGD_UVD_SUMSQ_WS_BYTES"]) == _lib.UVD_SUMSQ_WS_BYTES
    assert (int(consts["PSGD_DTYPE_F32"]), int(consts["PSGD_DTYPE_BF16"]), int(consts["PSGD_DTYPE_F16"])) == \
        (_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16)


def test_argument_checks(lib):
    """null pointers, k < 0, nchunks < 0 and unknown dtypes: PSGD_ERR_BAD_ARG (-1) with no device present"""
    BAD = _lib.PSGD_ERR_BAD_ARG
    assert BAD == -1
    segs, vsegs, chunks, out, x, pre, sq, ws = (0x10000 * k for k in range(1, 9))      # never dereferenced: the checks fail first
    pack, sumsq, upd = lib.psgd_uvd_pack_f32, lib.psgd_uvd_sumsq_f32, lib.psgd_uvd_param_update_multi
    assert pack(None, 3, chunks, 5, 0, 1.0, out, None) == BAD
    assert pack(segs, 3, None, 5, 0, 1.0, out, None) == BAD
    assert pack(segs, 3, chunks, 5, 0, 1.0, None, None) == BAD
    assert pack(segs, -1, chunks, 5, 0, 1.0, out, None) == BAD
    assert pack(segs, 3, chunks, -5, 0, 1.0, out, None) == BAD
    assert pack(segs, 3, chunks, 5, 3, 1.0, out, None) == BAD
    assert pack(segs, 3, chunks, 5, -1, 1.0, out, None) == BAD
    assert pack(segs, 3, chunks, 0, 1, 1.0, out, None) == _lib.PSGD_OK               # no chunk: nothing to launch
    assert sumsq(None, 10, sq, ws, 8192, None) == BAD
    assert sumsq(x, 10, None, ws, 8192, None) == BAD
    assert sumsq(x, 10, sq, None, 8192, None) == BAD
    assert sumsq(x, -1, sq, ws, 8192, None) == BAD
    assert sumsq(x, 10, sq, ws, 8191, None) == _lib.PSGD_ERR_WORKSPACE
    assert sumsq(x, 10, sq, ws + 4, 8192, None) == _lib.PSGD_ERR_WORKSPACE
    tail = (0.1, None, 0.0, 1e-38, None)
    assert upd(None, None, 3, chunks, 5, 0, pre, *tail) == BAD
    assert upd(segs, None, 3, None, 5, 0, pre, *tail) == BAD
    assert upd(segs, None, -3, chunks, 5, 0, pre, *tail) == BAD
    assert upd(segs, None, 3, chunks, -1, 0, pre, *tail) == BAD
    assert upd(segs, None, 3, chunks, 5, 7, pre, *tail) == BAD
    assert upd(segs, None, 3, chunks, 5, 0, None, *tail) == BAD                      # neither a gradient nor vs
    assert upd(segs, vsegs, 3, chunks, 5, 0, None, 0.1, sq, 1.0, 1e-38, None) == BAD  # a clip norm without a gradient
    assert upd(segs, vsegs, 3, chunks, 0, 2, pre, *tail) == _lib.PSGD_OK


def _check_cover(sizes):
    from psgd_tf_amd.preconditioned_stochastic_gradient_descent import uvd_tail_chunks
    C = _lib.UVD_TAIL_CHUNK
    table = uvd_tail_chunks(sizes)
    assert table.dtype == np.int64 and table.ndim == 2 and table.shape[1] == 2
    starts = np.cumsum(sizes) - np.asarray(sizes)
    hits = np.zeros(int(np.sum(sizes)), dtype=np.int32)
    for seg, off in table.tolist():
        assert 0 <= seg < len(sizes) and 0 <= off < sizes[seg] and off % C == 0
        n = min(C, sizes[seg] - off)                      # what the kernels take: never past the end of the segment
        assert n >= 1
        hits[starts[seg] + off:starts[seg] + off + n] += 1
    assert (hits == 1).all()
    assert (np.diff(table[:, 0]) >= 0).all()              # segments in order
    assert table.shape[0] == sum(-(-n // C) for n in sizes)


@pytest.mark.parametrize("sizes", [[1], [0, 5, 0], [3, 7, 4097], None])
def test_chunk_table_covers_every_element_once(sizes):
    if sizes is None:
        sizes = np.random.default_rng(0).integers(0, 70_002, 300).tolist()
        sizes[17], sizes[200] = 0, 70_001
    _check_cover(sizes)


def test_chunk_table_edges():
    from psgd_tf_amd.preconditioned_stochastic_gradient_descent import uvd_tail_chunks
    C = _lib.UVD_TAIL_CHUNK
    assert uvd_tail_chunks([]).shape == (0, 2) and uvd_tail_chunks([0, 0]).shape == (0, 2)
    for n in (C - 1, C, C + 1, 2 * C):
        _check_cover([n])
    with pytest.raises(ValueError):
        uvd_tail_chunks([3, -1])


def test_step_tail_value_is_checked_before_anything_is_allocated():
    import torch
    from psgd_tf_amd.preconditioned_stochastic_gradient_descent import UVd
    with pytest.raises(ValueError, match="step_tail"):
        UVd([torch.zeros(3, requires_grad=True)], step_tail="foreach")
