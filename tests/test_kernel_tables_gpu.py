"""Every row of the seven kernel tables (csrc/kernel_table.h) is ready to launch after its family's attribute setup: the function reports at least
the row's dynamic LDS, and no row asks for more than the 160 KB of a CU.  No kernel is launched."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

# (template, instantiations) in the order of ns2vc_debug_kernel_table's `family`: the counts tests/test_kernel_tables_cpu.py finds in the device code
FAMILIES = [("gemm2_kernel", 24), ("gemm4_kernel", 72), ("conv3ts_kernel", 70), ("attn_kernel", 40), ("ffn_kernel", 20), ("geglu_kernel", 4),
            ("rowchain_kernel", 40)]


@pytest.mark.parametrize("family", range(len(FAMILIES)), ids=[f[0] for f in FAMILIES])
def test_every_row_has_its_lds_attribute(family):
    from ns2vc_amd import _lib
    lib = _lib.load()
    rows, unready = C.c_int(-1), C.c_int(-1)
    assert lib.ns2vc_debug_kernel_table(family, C.byref(rows), C.byref(unready)) == 0
    assert rows.value == FAMILIES[family][1]
    assert unready.value == 0
