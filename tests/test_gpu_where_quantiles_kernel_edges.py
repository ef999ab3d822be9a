"""GPU: the quantile kernels (csrc/quant_kernels.h) at their edges. The cases are quant_model.edge_cases: values and mask bits laid out BY INDEX POSITION
(index_ids gives the position order, put_rows writes the columns through it), at most 2 * 10^5 rows each. Before a case is asked of the device, the sequential
stand-in (quant_model.select) runs over the layout the index REALLY has and the case's tags are asserted on its trace — digit passes and the last digit's width,
NP per pass, the bin of every rank, what the waves of the digit sweep see, bins flushed by two workgroups — so a case that no longer reaches its path fails
here instead of passing for nothing. The device's bytes are then compared with the stand-in's records and with numpy.sort's.

Four forms: the measure is the base field on its 4-byte column (E = 4, spans up to 32 bits) or on its 8-byte column (E = 2, up to 54 bits), or a probed
field, whose digit sweeps read the 8-byte value scratch (E = 2) behind a pass 0 over either column width."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bmx
import quant_model as qm
import where_agg_model as wam
from oracle import streams

WIDE = 2**40


@pytest.mark.parametrize("probe", [False, True], ids=["column", "probed"])
@pytest.mark.parametrize("wide", [False, True], ids=["int32", "int64"])
def test_kernel_edges(wide, probe):
    E = 2 if (wide or probe) else 4                                  # values per load of the digit sweeps
    cases = qm.edge_cases(E, 54 if E == 2 else 32)
    geom = qm.Geom(E)
    total = sum(len(c[1]) for c in cases)
    ids, fields = [], []
    for k, (name, v, bits, qs, check) in enumerate(cases):
        ids.append(wam.node_ids(len(v), 70000 * (k + 1)))
        fields.append(tuple(streams.fnv1a32("quant.edge.%s.%d" % (s, k)) for s in ("base", "bit", "measure")))
    with bmx.Engine(8 * total) as e:
        # the base rows first (a wide value where the int64 column is wanted), so that every index has its positions
        e.load_rows(np.concatenate(ids), np.concatenate([np.full(len(i), f[0], np.uint32) for i, f in zip(ids, fields)]), np.full(total, 1, np.int64),
                    np.full(total, WIDE if wide else 0, np.int64))
        order = [e.index_ids(f[0]) for f in fields]
        # the columns by position
        cols = []
        laid = []
        for (name, v, bits, qs, check), pos_ids, f in zip(cases, order, fields):
            assert len(pos_ids) == len(v), name
            if probe:
                base = np.arange(len(v), dtype=np.int64) % 100 + (WIDE if wide else 0)
                cols.append((pos_ids, f[2], v))
            else:
                shift = WIDE if wide and np.abs(v).max() < 2**31 else 0          # small values move up into the int64 column's own range
                base = v + shift; v = base
                assert wide or (base.min() > -(2**31) and base.max() < 2**31), name
            cols.append((pos_ids, f[0], base)); cols.append((pos_ids, f[1], bits.astype(np.int64)))
            laid.append(v)
        e.put_rows(np.concatenate([c[0] for c in cols]), np.concatenate([np.full(len(c[0]), c[1], np.uint32) for c in cols]), np.full(sum(len(c[0]) for c in cols), 2, np.int64),
                   np.concatenate([c[2] for c in cols]))
        for (name, _, bits, qs, check), pos_ids, f, v in zip(cases, order, fields, laid):
            assert np.array_equal(e.index_ids(f[0]), pos_ids), "the rows kept their positions"
            want, trace = qm.select(v, bits, qs, geom)
            check(trace)
            brute, mn, mx = qm.records(v[bits], qs)
            assert want.tobytes() == brute.tobytes(), name
            recs, res = qm.raw(e, f[0], [[(f[1], 1, 1)]], f[2] if probe else f[0], qs)
            assert recs.tobytes() == want.tobytes(), (name, recs, want)
            assert (int(res["n_match"]), int(res["n"]), int(res["min"]), int(res["max"])) == (int(bits.sum()), int(bits.sum()), mn, mx), name
