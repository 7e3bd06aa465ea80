"""k_trace's loop-carried ray state is not copied per trip: a static check of the gfx950 assembly (no GPU; one device-side
compile of csrc/pt_trace.hip with the Makefile's flags, through scripts/isa_report.py).

Before round 5 trace_chunk's outer loop had two exits and a `continue`; the register coalescer then copied the lane's whole
ray state (20-24 VGPRs) into a second register set at the top of every trip and back before the node walk.  PARENT holds
what that commit (a719c61) measured per instantiation <COUNT, RESUME, TOP, PRIMARY>, with
    python scripts/isa_report.py --no-blocks --filter k_trace
(hipcc of ROCm 7.2, clang 22, HIPFLAGS of csrc/Makefile): VGPR-to-VGPR copies (`v_mov_b32 vA, vB`) and vgpr_spill_count.
With one exit the copies are 35-50 against the parent's 212-315, so "at most half of the parent's" separates the two
regimes with room for compiler drift on either side.  No kernel may take more than 64 VGPRs (eight waves per SIMD) or spill
more VGPRs than the parent did.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_report                                                  # noqa: E402

#                    copies, vgpr_spill_count at the parent commit
PARENT = {"k_trace<1,0,0,0>": (315, 56),
          "k_trace<0,0,1,1>": (264, 11),
          "k_trace<0,0,1,0>": (256, 2),
          "k_trace<0,0,0,1>": (265, 11),
          "k_trace<0,0,0,0>": (258, 2),
          "k_trace<0,1,0,1>": (218, 0),
          "k_trace<0,1,0,0>": (212, 0)}
MAX_VGPRS = 64

_KERNELS = {}


def trace_kernels():
    if not _KERNELS:
        src = os.path.join(ROOT, "path_tracing_amd", "csrc", "pt_trace.hip")
        _KERNELS.update({k["name"]: k for k in isa_report.report(src) if k["name"].startswith("k_trace<")})
    return _KERNELS


needs_hipcc = pytest.mark.skipif(isa_report.find_hipcc() is None, reason="hipcc not found: the assembly cannot be produced")


@needs_hipcc
def test_every_instantiation_is_there():
    assert sorted(trace_kernels()) == sorted(PARENT)


@needs_hipcc
@pytest.mark.parametrize("name", list(PARENT))
def test_no_per_trip_copies_of_the_ray_state(name):
    k = trace_kernels()[name]
    copies, spills = PARENT[name]
    print("%s: %d VALU, %d copies (parent %d), %s VGPRs, %s VGPRs spilled (parent %d), %s SGPRs spilled" % (
        name, k["counts"]["valu"], k["counts"]["copies"], copies, k["meta"]["vgpr_count"], k["meta"]["vgpr_spill_count"], spills,
        k["meta"]["sgpr_spill_count"]))
    assert k["counts"]["valu"] > 500                               # the parser saw the kernel's body
    assert 2 * k["counts"]["copies"] <= copies
    assert k["meta"]["vgpr_count"] <= MAX_VGPRS
    assert k["meta"]["vgpr_spill_count"] <= spills


def test_the_parser_counts_what_it_says():
    """classify() and parse() on a hand-written listing: no compiler needed."""
    asm = "\n".join([
        "\t.globl\t_Z3fooILb1ELb0EEvPf", "_Z3fooILb1ELb0EEvPf:", "; %bb.0:",
        "\ts_load_dwordx2 s[0:1], s[4:5], 0x0", "\tv_mov_b32_e32 v1, v0", "\tv_mov_b32_e32 v2, 0", "\ts_waitcnt lgkmcnt(0)",
        ".LBB0_1:                                ; =>This Inner Loop Header: Depth=1",
        "\tv_add_f32_e32 v1, v1, v2", "\tv_mov_b32_e32 v3, v1", "\tv_readlane_b32 s6, v40, 3", "\ts_add_u32 s2, s2, 1",
        "\tscratch_load_dword v4, off, off offset:4", "\ts_cbranch_scc1 .LBB0_1",
        "; %bb.2:", "\tv_mov_b32_e32 v5, s0", "\ts_endpgm", ".Lfunc_end0:",
        "amdhsa.kernels:", "  - .agpr_count:     0", "    .name:           _Z3fooILb1ELb0EEvPf", "    .sgpr_count:     12",
        "    .sgpr_spill_count: 1", "    .vgpr_count:     41", "    .vgpr_spill_count: 1", "amdhsa.target:   amdgcn-amd-amdhsa--gfx950"])
    (k,) = isa_report.parse(asm)
    assert k["name"] == "foo<1,0>"
    assert k["counts"] == {"valu": 6, "salu": 1, "copies": 2, "lane": 1, "scratch": 1}
    assert k["meta"] == {"agpr_count": 0, "sgpr_count": 12, "sgpr_spill_count": 1, "vgpr_count": 41, "vgpr_spill_count": 1}
    assert [(b["label"], b["depth"], b["counts"]["valu"]) for b in k["blocks"]] == [("entry", 0, 2), (".LBB0_1", 1, 3), ("%bb.2", 0, 1)]
