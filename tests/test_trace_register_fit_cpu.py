"""The timed k_trace instantiations keep their register fit: eight waves per SIMD (at most 64 VGPRs), no VGPR spilled and no
scratch instruction.  A static check of the gfx950 assembly (no GPU; scripts/isa_report.py, as tests/test_trace_isa_cpu.py).

The benchmark's render runs <COUNT, RESUME, TOP, PRIMARY> = <0,0,1,0> (first launch, the tree's top in LDS), <0,0,0,0>
(first launch of a budget above kTopLevels) and <0,1,0,0> (resume launch) past iteration 0.  The first two write a ray they
set aside as a record (three stores from registers that are live anyway), the third starts a ray from one (three loads of
one record in place of four gathers); neither may cost the kernel its occupancy.  Registers and spills only: what the instructions are is
tests/test_trace_isa_cpu.py's business.
"""
import pytest

import test_trace_isa_cpu as isa

TIMED = ["k_trace<0,0,1,0>", "k_trace<0,0,0,0>", "k_trace<0,1,0,0>"]


@isa.needs_hipcc
@pytest.mark.parametrize("name", TIMED)
def test_timed_instantiations_fit_eight_waves(name):
    k = isa.trace_kernels()[name]
    print("%s: %s VGPRs, %s spilled, %d scratch instructions, %s SGPRs, %s spilled to lanes" % (
        name, k["meta"]["vgpr_count"], k["meta"]["vgpr_spill_count"], k["counts"]["scratch"], k["meta"]["sgpr_count"], k["meta"]["sgpr_spill_count"]))
    assert k["counts"]["valu"] > 500                               # the parser saw the kernel's body
    assert k["meta"]["vgpr_count"] <= isa.MAX_VGPRS
    assert k["meta"]["vgpr_spill_count"] == 0
    assert k["counts"]["scratch"] == 0
