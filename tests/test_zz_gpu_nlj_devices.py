"""dfgpu_nested_loop_join refuses tables that live on different devices.  Needs two GPUs in one process, like
tests/test_zz_gpu_multi_device.py (whose set-up this follows: named test_zz_* so that it comes last, self-skipping on a box with one GPU)."""
import ctypes as C

import pytest

from tests import nlj_cases as NC

pytestmark = pytest.mark.gpu


def test_tables_on_different_devices_are_refused():
    from datafusion_amd import _lib, ops
    from datafusion_amd.table import DeviceTable
    lib = _lib.load()
    n = C.c_int(0)
    assert lib.dfgpu_device_count(C.byref(n)) == 0
    if n.value < 2:
        pytest.skip(f"{n.value} GPU visible: tables on two devices need two")
    _lib.init(0)
    _lib.check(lib.dfgpu_init((C.c_int * 2)(0, 1), 2))
    left, right = NC.null_tables(5, 4)
    dl = DeviceTable.from_arrow(left)
    _lib.check(lib.dfgpu_set_device(1))
    try:
        dr = DeviceTable.from_arrow(right)
    finally:
        _lib.check(lib.dfgpu_set_device(0))
    for jt in ("Inner", "LeftAnti"):
        with pytest.raises(_lib.DfgpuError, match="lives on another device"):
            ops.nested_loop_join(dl, dr, jt, None)
    _lib.check(lib.dfgpu_set_device(0))
    for t in (dl, dr):
        t.free()
