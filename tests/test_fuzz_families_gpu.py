"""A fixed number of randomised cases per family (tests/fuzz_gpu.py: run_cases) for the families the timed rotation of
tests/test_fuzz_gpu.py does not reach, or reaches too thinly: the dense preconditioner, the bf16-state UVd kernels, the sparse-LU
update against the oracle, and the fp32 UVd calls with a matrix g at every rank.  Which cases run depends on the seed and the count
alone, never on the speed of the box.  Each count covers every residue of the family's `it % k` switches at least twice; what the
cases then were is asserted from the names the family reports.  No case may lean on fuzz_uvd's sensitivity relaxation: its message
must not appear."""
import time

import pytest

pytestmark = pytest.mark.gpu

SEED = 20250
RELAXED = "the fp64 update moves"       # fuzz_uvd's message when it widens its bar


def _run(family, count, capsys):
    from tests import fuzz_gpu
    log = []
    t0 = time.time()
    cases, bad, worst = fuzz_gpu.run_cases([family], count, SEED, log)
    out = capsys.readouterr().out
    with capsys.disabled():
        print("\n%s: %d cases in %.1f s, worst %.3e (%s)" % (family, cases, time.time() - t0, *worst[family]))
    assert cases == count == len(log)
    assert not bad, bad[:5]
    assert RELAXED not in out, out
    assert all(name.split()[0] == family for name, _, _ in log)
    return [name.split() for name, _, _ in log]


def _num(words, key):
    return int(next(w for w in words if w.startswith(key))[len(key):])


def _gram_cases(names):
    """every fifth case (it % 5 == 2; names are in the order of it) of rank 2 and above is a problem of make_uvd_problem_with_gram, and
    no other: at least three, each kind of the rotation met"""
    from tests import fuzz_gpu
    kinds = {it: x[len("gram-"):] for it, w in enumerate(names) for x in w if x.startswith("gram-")}
    assert sorted(kinds) == [it for it, w in enumerate(names) if it % 5 == 2 and _num(w, "r=") > 1], sorted(kinds)
    assert len(kinds) >= max(3, len(names) // 5 - 2), kinds
    assert set(kinds.values()) == set(fuzz_gpu.GRAM_KINDS), kinds


def test_dense(hip_lib, capsys):
    """36 cases: it % 2 (upper / full), it % 3 with (it // 3) % 4 (the four edge classes, three cases each), it % 4 (unaligned Q),
    one scaled case in every three."""
    from tests import fuzz_gpu
    del fuzz_gpu.DENSE_RATIOS[:]
    names = _run("dense", 36, capsys)
    for cls in ("edge64", "edge256", "edge1024", "route64"):
        assert sum(cls in w for w in names) >= 2, cls
    big_unaligned = [w for w in names if "unaligned" in w and _num(w, "N=") > 64]
    assert len(big_unaligned) >= 2 and all(_num(w, "N=") % 4 == 0 for w in big_unaligned)
    for word in ("upper", "full", "c=0.3", "c=1.0", "c=2.0", "step=0.01", "step=0.10"):
        assert sum(word in w for w in names) >= 2, word
    assert sum(any(x.startswith("s=") for x in w) for w in names) >= 2
    assert len(fuzz_gpu.DENSE_RATIOS) == sum("c=2.0" in w for w in names)
    with capsys.disabled():
        for row in fuzz_gpu.DENSE_RATIOS:
            print("  err_native / err_torch  Q %.2f  increment %.2f  apply %.2f  (%s)" % (row[1:] + row[:1]))


def test_uvd_bf16(hip_lib, capsys):
    """64 cases: it % 2 (U / V), (it // 2) % 2 (rounding), (it // 4) % 2 (fused / two calls), it % 5 (balance), it % 3 with
    (it // 3) % 3 (three tile multiples), it % 4 (N to 400 000), it % 5 == 2 (13 slots for problems with a chosen Gram,
    tests/uvd_cases.py, at every rank but 1; hard bars like the rest).  The rank is a uniform draw: this seed meets 24 of the 32
    ranks (the others: 2, 3, 6, 10, 17, 21, 25, 29; profiles/fuzz_families.txt), and a change of seed or generator may not meet
    fewer."""
    names = _run("uvd-bf16", 64, capsys)
    for word in ("U", "V", "bal", "nearest", "stochastic", "fused", "two-call", "edge64", "edge256"):
        assert sum(word in w for w in names) >= 2, word
    assert sum(any(x.startswith("edgeTR") for x in w) for w in names) >= 2
    assert sum(_num(w, "N=") > 20000 for w in names) >= 2
    ranks = {_num(w, "r=") for w in names}
    with capsys.disabled():
        print("  ranks met: %d of 32, missing %s" % (len(ranks), sorted(set(range(1, 33)) - ranks)))
    assert min(ranks) >= 1 and max(ranks) <= 32 and len(ranks) >= 24, sorted(ranks)
    _gram_cases(names)


def test_splu(hip_lib, capsys):
    """30 cases: it % 5 (ranks above 32), it % 4 (N to 300 000)."""
    names = _run("splu", 30, capsys)
    assert sum(_num(w, "r=") > 32 for w in names) >= 2 and sum(_num(w, "r=") <= 32 for w in names) >= 2
    assert sum(_num(w, "N=") > 20000 for w in names) >= 2


def test_uvd(hip_lib, capsys):
    """30 cases: it % 15 (ranks above 32), it % 2 (U / V, and the matrix g on the even ones), it % 3, it % 4, it % 5 (== 0: balance;
    == 2: six slots for problems with a chosen Gram, tests/uvd_cases.py, at every rank but 1, never with the sensitivity
    relaxation)."""
    names = _run("uvd", 30, capsys)
    assert sum(_num(w, "r=") > 32 for w in names) >= 2 and sum(_num(w, "r=") <= 32 for w in names) >= 15
    _gram_cases(names)
