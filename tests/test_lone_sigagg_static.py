"""The lone sigagg route's kernels in the built library, read on the CPU: they are in the runtime's
kernel table and in the code object, their private segments fit the scratch budget, and the stage-2 kernel's LDS lets
four of its workgroups share a CU."""
import ctypes
import os

import pytest

from charon_amd import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "charon_amd", "libhipbls.so")
KERNELS = ("k_tv_prep8", "k_tv_pair_lq16", "k_tagg_sum8")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libhipbls.so not built (run __graft_entry__.build())")


@pytest.fixture(scope="module")
def rows():
    return {r[0]: r for r in codeobj.resource_table(LIB) if r[0] in KERNELS}


def test_kernel_table_and_code_object_hold_the_route(rows):
    lib = ctypes.CDLL(LIB)
    lib.hipbls_kernel_names.restype = ctypes.c_char_p
    table = lib.hipbls_kernel_names().decode().split()
    for k in KERNELS:
        assert k in table, k
        assert k in rows, k


def test_private_segments_within_budget(rows):
    for k in KERNELS:
        name, scratch, vgpr, lds = rows[k]
        assert 0 < scratch <= codeobj.PRIVATE_SEGMENT_BUDGET, (k, scratch)


def test_stage_two_lds_leaves_four_workgroups_per_cu(rows):
    """The sum is a chain of quad additions in registers, so the only LDS is the race words every latency kernel
    declares; in any case four workgroups must fit a CU's 160 KiB."""
    for k in ("k_tv_pair_lq16", "k_tagg_sum8"):
        lds = rows[k][3]
        assert 4 * lds <= 160 * 1024, (k, lds)
