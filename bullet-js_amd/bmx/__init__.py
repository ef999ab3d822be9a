"""bmx — ctypes binding of libbmx.so (include/bmx.h), the MI355X CRDT-merge / index-scan engine.

This is the Python-side driver used by tests and bench.py. The product surface is the C ABI and the
N-API/JS host (bullet-js_amd/js); nothing here computes anything on the CPU: every call goes to the
HIP library and raises BmxError if it (or a GPU) is missing.

The package is its modules' names under one roof: _abi (constants, records, signatures, load_library), _results (what queries return, the host-side
merges), _queries (how each query's arguments are marshalled, once), engine / comm / vc (the three handle classes); sharded, replica and synth build on it.
Every public name of those modules is a name of the package, and so are the helpers below that tests and micro-benchmarks use.
"""
from ._abi import *          # noqa: F401,F403
from ._abi import _PKG, _np, _ptr, _ref          # noqa: F401
from ._results import *      # noqa: F401,F403
from ._results import _group_fold          # noqa: F401
from ._queries import *      # noqa: F401,F403
from ._queries import (_agg_args, _first_buffers, _first_tail, _group_tail, _gtop_buffers, _gtop_tail, _join_pairs, _jrows_flags, _jrows_pairs, _mgroup_keys,          # noqa: F401
                       _quant_tail, _rows_buffers, _rows_fields, _semi_values, _top_args, _upd_args, _where_agg_tail, _where_args, _where_entries, _where_top_tail)
from .engine import *        # noqa: F401,F403
from .engine import _bucket_words, _mix64          # noqa: F401
from .comm import *          # noqa: F401,F403
from .vc import *            # noqa: F401,F403

