"""GpuQuery.countBy / aggregateWhere and DeviceGraph.scanAggregate through the N-API addon (bullet-js_amd/js/test/query_aggregate.js): the reference's example
dataset, per-value counts against the fixture's equals / range answers, sum / min / max against a plain reduce, a sum beyond 2^53 as a BigInt."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "bullet-js_amd", "js", "test")
NODE = shutil.which("node")

needs_node = pytest.mark.skipif(NODE is None, reason="node is not installed on this box")


@needs_node
def test_addon_exports_the_aggregate_calls():
    import __graft_entry__ as g
    g.build()
    addon = os.path.join(ROOT, "bullet-js_amd", "bmx.node")
    code = ("const b=require(%r); for (const k of ['scanAggregate','commScanAggregate']) if (typeof b[k]!=='function') { console.log('missing',k); process.exit(3); }"
            "const G=require(%r); if (typeof G.prototype.scanAggregate!=='function') process.exit(4);"
            "const Q=require(%r); for (const k of ['aggregateWhere','countBy','map','filter','find']) if (typeof Q.prototype[k]!=='function') process.exit(5); console.log('addon ok');"
            % (addon, os.path.join(ROOT, "bullet-js_amd", "js", "device-graph.js"), os.path.join(ROOT, "bullet-js_amd", "js", "gpu-query.js")))
    out = subprocess.run([NODE, "-e", code], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "addon ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@needs_node
def test_query_aggregate_through_napi():
    out = subprocess.run([NODE, os.path.join(JS, "query_aggregate.js"), os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "query_aggregate ok" in out.stdout
