"""GpuQuery.whereAggregate / whereTop and DeviceGraph.whereAggregate / whereTop through the N-API addon (bullet-js_amd/js/test/query_where_agg.js): Example 8
of the reference's docs/querying.md grouped by role codes, an OR of two equalities paged — against filter(path, fn) followed by a reduce / a sort written out
by hand: whereTop over host indexes (strings, booleans) anywhere, both calls over integer indexes on the device where there is one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "bullet-js_amd", "js", "test")
NODE = shutil.which("node")

needs_node = pytest.mark.skipif(NODE is None, reason="node is not installed on this box")


@needs_node
def test_addon_exports_the_where_agg_calls():
    import __graft_entry__ as g
    g.build()
    addon = os.path.join(ROOT, "bullet-js_amd", "bmx.node")
    code = ("const b=require(%r); for (const k of ['whereAggregate','whereTop','commWhereAggregate','commWhereTop']) if (typeof b[k]!=='function') { console.log('missing',k); process.exit(3); }"
            "const G=require(%r); for (const k of ['whereAggregate','whereTop']) if (typeof G.prototype[k]!=='function') process.exit(4);"
            "const Q=require(%r); for (const k of ['whereAggregate','whereTop','where']) if (typeof Q.prototype[k]!=='function') process.exit(5); console.log('addon ok');"
            % (addon, os.path.join(ROOT, "bullet-js_amd", "js", "device-graph.js"), os.path.join(ROOT, "bullet-js_amd", "js", "gpu-query.js")))
    out = subprocess.run([NODE, "-e", code], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "addon ok" in out.stdout, out.stdout + out.stderr


@needs_node
def test_query_where_agg_on_host_indexes():
    out = subprocess.run([NODE, os.path.join(JS, "query_where_agg.js"), os.path.join(ROOT, "tests", "golden"), "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "query_where_agg ok" in out.stdout and "host indexes only" in out.stdout


@pytest.mark.gpu
@needs_node
def test_query_where_agg_through_napi():
    out = subprocess.run([NODE, os.path.join(JS, "query_where_agg.js"), os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "query_where_agg ok" in out.stdout and "host indexes only" not in out.stdout
