"""tbls_init / tbls_shutdown / tbls_init in one process (tools/lifecycle_probe.py,
a child process: the test session's own library state is never shut down).
Every buffer, stream and event of a context is created, used, destroyed with
its context and created again: two shared library devices with a key table and
a batch, shutdown, one device without a table, the same batch accepted and a
tampered one rejected, shutdown, a clean exit."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_init_shutdown_init_verifies_again():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lifecycle_probe.py")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ), cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, p.stdout[-2000:] + p.stderr[-2000:]
    r = json.loads(lines[-1])
    print(r)
    assert r["devices_first"] == 2 and r["table_first"] == 8 and r["valid_first"] is True
    assert r["devices_after_shutdown"] == 0
    assert r["devices_second"] == 1 and r["table_second"] == 0
    assert r["valid_second"] is True and r["tampered_second"] is False
    assert r["devices_end"] == 0
    assert p.returncode == 0, p.stderr[-2000:]
