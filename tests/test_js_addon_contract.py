"""The N-API addon's contract (bullet-js_amd/js/test/addon_contract.js): exported names and constants, the class, text and .code of its errors, result
types, closed and foreign handles, and issue order across asynchronous merges. The host half needs no device; the device half runs the engine, the
vector-clock table and communicators of one and two logical shards."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "bullet-js_amd", "js", "test", "addon_contract.js")
NODE = shutil.which("node")

needs_node = pytest.mark.skipif(NODE is None, reason="node is not installed on this box")


@needs_node
def test_addon_contract_on_the_host():
    import __graft_entry__ as g
    g.build()
    out = subprocess.run([NODE, SCRIPT, "host"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "addon_contract ok (host" in out.stdout


@pytest.mark.gpu
@needs_node
def test_addon_contract_on_the_device():
    out = subprocess.run([NODE, SCRIPT, "gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "addon_contract ok (gpu" in out.stdout and "handles of another kind checked" in out.stdout
