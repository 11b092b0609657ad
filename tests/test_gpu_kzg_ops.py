"""GPU parity of the KZG kernels' scalar side -- Fr (tb_fr.h), the GLV split and
the GLV scalar multiplication (tb_glv.h) -- through the test library's
k_test_ops_c, against Python integers and the oracle.  The same cases and
checks as tests/test_kzg_ops.py (tests/kzg_cases.py)."""

import pytest

from tests import kzg_cases as C
from tests.opcodec import load_test_lib, run_ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    L = load_test_lib()
    return lambda op, recs: run_ops(L.tbls_test_ops, op, recs)


@pytest.mark.parametrize("check", C.CHECKS, ids=lambda f: f.__name__[6:])
def test_kzg_op(run, check):
    check(run)
