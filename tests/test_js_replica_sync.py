"""DeviceGraph.digest / exportRows through the N-API addon (bullet-js_amd/js/test/replica_sync.js): two graphs, digest totals against the rowDigest sum of
dumpRows(), one graph's export merged into the other with BMX_INSERT_DELTA, equal digests afterwards; single contexts and 4-shard communicators."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "bullet-js_amd", "js", "test")
NODE = shutil.which("node")

needs_node = pytest.mark.skipif(NODE is None, reason="node is not installed on this box")


@needs_node
def test_addon_exports_the_reconciliation_calls():
    import __graft_entry__ as g
    g.build()
    addon = os.path.join(ROOT, "bullet-js_amd", "bmx.node")
    code = ("const b=require(%r); for (const k of ['digest','exportRows','commDigest','commExportRows']) if (typeof b[k]!=='function') { console.log('missing',k); process.exit(3); }"
            "const G=require(%r); for (const k of ['digest','exportRows']) if (typeof G.prototype[k]!=='function') process.exit(4); console.log('addon ok');"
            % (addon, os.path.join(ROOT, "bullet-js_amd", "js", "device-graph.js")))
    out = subprocess.run([NODE, "-e", code], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "addon ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@needs_node
def test_replica_sync_through_napi():
    out = subprocess.run([NODE, os.path.join(JS, "replica_sync.js")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "replica_sync ok" in out.stdout
