import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "mkl_reproducible: runs in a child interpreter on MKL's reproducible code path "
                                       "(MKL_CBWR=COMPATIBLE, the path tests/golden/make_golden.py generates the fixtures on)")


@pytest.hookimpl(tryfirst=True)
def pytest_pyfunc_call(pyfuncitem):
    """The CPU oracle against the reference's fixtures, to 2e-5: the sharp-weight fixtures amplify a 1-ulp difference between
    MKL's per-CPU sgemm kernels (AVX-512 on Intel hosts, others on AMD hosts) into 1e-2 at a few fine samples, so these tests take
    the one path that gives the same bits on every x86 host.  MKL reads the setting once, at its first call: a child process per
    test, the rest of the suite keeps the host's own path."""
    if pyfuncitem.get_closest_marker("mkl_reproducible") is None or os.environ.get("MKL_CBWR") == "COMPATIBLE":
        return None
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-m", "pytest", "-q", "-p", "no:cacheprovider", pyfuncitem.nodeid]
    r = subprocess.run(cmd, cwd=str(pyfuncitem.config.rootpath), env=dict(os.environ, MKL_CBWR="COMPATIBLE"),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and re.search(r"^1 passed\b", r.stdout, re.M), r.stdout[-4000:] + r.stderr[-2000:]
    return True
