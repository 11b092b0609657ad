"""CPU checks of the KZG kernels' scalar side -- Fr (tb_fr.h), the GLV split and
the GLV scalar multiplication (tb_glv.h) -- through the host build of the test
ops (tests/native/tb_testops.h, hostsim), against Python integers and the
oracle.  The same cases and checks as tests/test_gpu_kzg_ops.py
(tests/kzg_cases.py).  Test infrastructure only: the product has no CPU path."""

import ctypes

import pytest

from tests import kzg_cases as C
from tests.opcodec import run_ops


@pytest.fixture(scope="module")
def run():
    import __graft_entry__ as ge

    lib = ctypes.CDLL(ge.build_hostsim())
    fn = lib.tbls_hostsim_test_ops
    fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return lambda op, recs: run_ops(fn, op, recs)


@pytest.mark.parametrize("check", C.CHECKS, ids=lambda f: f.__name__[6:])
def test_kzg_op(run, check):
    check(run)


def test_glv_case_classes():
    """The GLV_SPLIT inputs reach both the uncorrected and the corrected branch
    (a random scalar is a multiple of mu with probability about 2^-128)."""
    classes = [C.glv_corrections(k) for k in C.glv_cases()]
    assert classes.count(0) >= 40 and classes.count(1) >= 40 and set(classes) == {0, 1}
    assert all(C.glv_corrections(j * C.MU) == 1 for j in (1, 2, C.MU - 1))
