"""The {field, clock: "data" | "deleted" | "any"} term of GpuQuery.where / whereAggregate / whereTop / whereRows (bullet-js_amd/js/test/query_where_clock.js): a range
over the clock of a field's row in its index, each form against a host filter over the clocks and states whereRows reports — over a host index anywhere, and
through the N-API addon on the device where there is one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "bullet-js_amd", "js", "test")
NODE = shutil.which("node")

needs_node = pytest.mark.skipif(NODE is None, reason="node is not installed on this box")


@needs_node
def test_query_where_clock_on_host_indexes():
    out = subprocess.run([NODE, os.path.join(JS, "query_where_clock.js"), os.path.join(ROOT, "tests", "golden"), "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "query_where_clock ok" in out.stdout and "host indexes only" in out.stdout


@pytest.mark.gpu
@needs_node
def test_query_where_clock_through_napi():
    out = subprocess.run([NODE, os.path.join(JS, "query_where_clock.js"), os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "query_where_clock ok" in out.stdout and "host indexes only" not in out.stdout
