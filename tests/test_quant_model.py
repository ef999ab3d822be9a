"""CPU: the sequential stand-in of the quantile kernels (quant_model.select: k_quant_init / k_quant_digit / k_quant_find of csrc/quant_kernels.h) against
brute force (numpy.sort + bmx.quant_rank), with the kernels' constants and with constants scaled down so that few rows reach every path; the rank rule; and
every tag the GPU kernel-edge tests assert before they ask the device is reachable by the cases they use."""
import numpy as np
import pytest

import bmx
import quant_model as qm
import where_agg_model as wam
from where_agg_model import DATA

SMALL = dict(digit_bits=3, threads=8, inflight=2, wave=4, find_threads=4, max_groups=3, rounds_per_group=2)


def test_rank_rule():
    for n in (1, 2, 3, 10, 11, 1000, 2**31):
        assert bmx.quant_rank(0, 1, n) == 0 and bmx.quant_rank(1, 1, n) == n - 1 and bmx.quant_rank(1, 2, n) == (n - 1) // 2 == bmx.quant_rank(2, 4, n)
    v = np.sort(np.random.default_rng(1).integers(-50, 50, 101))
    for num, den in ((1, 4), (3, 4), (95, 100), (99, 100), (1, 3)):
        assert v[bmx.quant_rank(num, den, len(v))] == np.percentile(v, 100.0 * num / den, method="lower")
    assert bmx.quant_rank(2**20, 2**20, 2**44) == 2**44 - 1
    for bad in ((1, 0, 5), (2, 1, 5), (-1, 2, 5), (1, 2**20 + 1, 5), (1, 2, 0)):
        with pytest.raises(ValueError):
            bmx.quant_rank(*bad)


def test_the_model_counts_what_the_header_says():
    """selection x the three cell states of the measure: absent and tombstoned measures count in n_match, not in n"""
    m = wam.Model(np.arange(1, 13, dtype=np.uint64))
    m.set(1, np.arange(12), np.arange(12))                   # base
    m.set(2, np.arange(0, 8), [5, 3, 9, 3, 7, 1, 3, 8]); m.tomb(2, [6, 7])
    recs, res = qm.quantiles(m, 1, [[(1, 2, 11)]], 2, [(0, 1), (1, 2), (1, 1), (1, 2)])
    assert (int(res["n_match"]), int(res["n"]), int(res["min"]), int(res["max"])) == (10, 4, 1, 9)     # nodes 2..5 hold data: 9 3 7 1
    assert recs.tolist() == [(1, 0, 0, 1), (3, 1, 1, 1), (9, 3, 3, 1), (3, 1, 1, 1)]
    recs, res = qm.quantiles(m, 1, [[(1, 8, 11)]], 2, [(1, 2)])
    assert recs.tolist() == [(0, 0, 0, 0)] and (int(res["n_match"]), int(res["n"]), int(res["min"]), int(res["max"])) == (4, 0, qm.I64MAX, qm.I64MIN)


@pytest.mark.parametrize("geom", [qm.Geom(4), qm.Geom(2), qm.Geom(4, **SMALL), qm.Geom(2, **SMALL)], ids=["E4", "E2", "E4 small", "E2 small"])
def test_the_stand_in_against_brute_force(geom):
    rng = np.random.default_rng(5 + geom.E + geom.digit_bits)
    for trial in range(60):
        n = int(rng.integers(1, 400))
        span = int(rng.integers(0, 55))
        lo = int(rng.integers(-(1 << 53) + 1, (1 << 53) - (1 << span))) if span < 54 else -(1 << 53) + 1
        v = lo + rng.integers(0, (1 << span) - (span == 54), n, endpoint=span < 54)
        if trial % 3 == 0:
            v[rng.random(n) < 0.5] = v[0]                    # a tie group
        bits = rng.random(n) < rng.choice([0.0, 0.1, 0.9, 1.0])
        qs = [(int(a), int(b)) for b in rng.integers(1, 50, int(rng.integers(1, 9))) for a in [rng.integers(0, b + 1)]]
        got, t = qm.select(v, bits, qs, geom)
        want, _, _ = qm.records(v[bits], qs)
        assert got.tobytes() == want.tobytes(), (trial, got, want)
        if bits.any():
            d = int(v[bits].max()) - int(v[bits].min())
            assert t.passes == (d.bit_length() + geom.digit_bits - 1) // geom.digit_bits and t.np[:1] == [1][:t.passes] and all(1 <= x <= len(set(qs)) for x in t.np)
        else:
            assert t.passes == 0 and not got.view(np.uint8).any()


@pytest.mark.parametrize("E,max_bits", [(4, 32), (2, 54)])
def test_every_tag_of_the_gpu_edge_cases_is_reachable(E, max_bits):
    names = []
    for name, v, bits, qs, check in qm.edge_cases(E, max_bits):
        got, t = qm.select(v, bits, qs, qm.Geom(E))
        check(t)
        want, _, _ = qm.records(v[bits], qs)
        assert got.tobytes() == want.tobytes(), name
        if max_bits == 32:
            assert v.min() > -(1 << 31) and v.max() < (1 << 31), name
        assert np.abs(v).max() <= (1 << 53) - 1, name
        names.append(name)
    spans = [int(x.split()[1]) for x in names if x.startswith("span")]
    assert {(s + 10) // 11 for s in spans} == set(range(0, 4 if max_bits == 32 else 6)), "every digit count"
    sizes = [int(x.split()[1]) for x in names if x.startswith("size")]
    assert any(qm.Geom(E).groups(n) == 2 for n in sizes) and any(n % E for n in sizes) and len(names) == len(set(names))
