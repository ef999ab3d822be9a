"""GpuQuery.whereRows and DeviceGraph.whereRows through the N-API addon (bullet-js_amd/js/test/query_where_rows.js): Example 8 of the reference's
docs/querying.md and an OR of two equalities, paged — against filter(path, fn) followed by a projection written out by hand: over host indexes (strings,
booleans) anywhere, over integer indexes on the device where there is one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "bullet-js_amd", "js", "test")
NODE = shutil.which("node")

needs_node = pytest.mark.skipif(NODE is None, reason="node is not installed on this box")


@needs_node
def test_addon_exports_the_where_rows_calls():
    import __graft_entry__ as g
    g.build()
    addon = os.path.join(ROOT, "bullet-js_amd", "bmx.node")
    code = ("const b=require(%r); for (const k of ['whereRows','commWhereRows']) if (typeof b[k]!=='function') { console.log('missing',k); process.exit(3); }"
            "const G=require(%r); if (typeof G.prototype.whereRows!=='function') process.exit(4);"
            "const Q=require(%r); if (typeof Q.prototype.whereRows!=='function') process.exit(5); console.log('addon ok');"
            % (addon, os.path.join(ROOT, "bullet-js_amd", "js", "device-graph.js"), os.path.join(ROOT, "bullet-js_amd", "js", "gpu-query.js")))
    out = subprocess.run([NODE, "-e", code], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "addon ok" in out.stdout, out.stdout + out.stderr


@needs_node
def test_query_where_rows_on_host_indexes():
    out = subprocess.run([NODE, os.path.join(JS, "query_where_rows.js"), os.path.join(ROOT, "tests", "golden"), "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "query_where_rows ok" in out.stdout and "host indexes only" in out.stdout


@pytest.mark.gpu
@needs_node
def test_query_where_rows_through_napi():
    out = subprocess.run([NODE, os.path.join(JS, "query_where_rows.js"), os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "query_where_rows ok" in out.stdout and "host indexes only" not in out.stdout
