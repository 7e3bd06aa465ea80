"""k_shade fills no register with a value nobody reads, and its unit-ball try is the short one: a static check of the gfx950
assembly (no GPU; one device-side compile of csrc/pt_shade.hip with the Makefile's flags, through scripts/isa_report.py).

Before round 7 the twenty next-event record words and `path` were initialised where they are declared, at the top of a
trip of the kernel's loop.  They are read under `if(nee)` only, but a default is a value, so the compiler set all of them to
zero in the loop's header block, again in the block behind the `i < count` test, and a few at a time at the joins of the
divergent branches further down.  PARENT holds what that commit (1056ac2) gave per instantiation <PRIMARY, STRIDED>, from
    python scripts/isa_report.py path_tracing_amd/csrc/pt_shade.hip --asm-out DIR
(hipcc of ROCm 7.2, clang 22, HIPFLAGS of csrc/Makefile) and trip_loop() below on the listing: the `v_mov_b32 vN, 0`
inside the trip loop, and how many of those sit in the two head blocks that every trip runs before any lane has loaded
anything (<0,0>: .LBB2_37 and .LBB2_41; <1,0>: .LBB0_37 and .LBB0_45, the block behind primary_ray; <0,1>: .LBB1_43 and
.LBB1_47).  With the words declared without initialisers and written only where `nee` is set, the head blocks' moves cannot
be there, so the bound is the parent's count minus its head blocks': 153, 175 and 153.  (Measured after the change: 53, 79
and 53 -- the joins further down lost theirs too; one of those left is the parallel-light record's n_pdf_light = 0.)

The try -- the innermost loop, three steps of the random stream and a dot product -- was 51 VALU instructions.  Each of its
three coordinates cost a convert and three float operations (times 2^-24, times 2, minus 1) and costs a convert and one
fused multiply-add now (tests/test_ball_coordinate_cpu.py: the same bits), six instructions fewer: at most 45.  (Measured:
43, and 9 quarter-rate integer multiplies against 10.)

Four workgroups of k_shade fit a compute unit's LDS, four waves per SIMD, so up to 512 / 4 = 128 VGPRs cost no occupancy:
every instantiation stays within them, with no scratch instruction and no spilled VGPR."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_report                                                  # noqa: E402

#                   zero moves in the trip loop, of which in its two head blocks, at the parent commit
PARENT = {"k_shade<1,0>": (212, 18 + 19),
          "k_shade<0,1>": (187, 15 + 19),
          "k_shade<0,0>": (192, 20 + 19)}
PARENT_TRY_VALU = 51
TRY_SAVED = 6                          # three coordinates, two float operations fewer each
MAX_VGPRS = 128

_SHADE = {}
_ZERO_MOVE = re.compile(r"^v_mov_b32(_e32)?\s+v\d+,\s*0\s*$")


def _count(code, *ops):
    return sum(c.startswith(ops) for c in code)


def trip_loop(blocks):
    """k_shade's trip loop in a kernel's isa_report.listing() and the unit-ball try in it: dict(try_block, header, blocks,
    zero_moves, zero_by_block).  The try is THE single-block loop that steps the random stream three times (three or more
    64-bit multiply-adds), converts three integers to floats and compares with 1.0 -- exactly one block of the kernel may
    look like that, or this raises.  The trip loop is the innermost loop around it, taken as the run of blocks from that
    loop's header to the last block whose note names the header.  zero_moves counts `v_mov_b32 vN, 0` in that run."""
    tries = [b for b in blocks if "Inner Loop Header" in b["note"] and _count(b["code"], "v_mad_u64_u32") >= 3
             and _count(b["code"], "v_cvt_f32_u32") == 3 and any(c.startswith("v_cmp") and " 1.0" in c for c in b["code"])]
    if len(tries) != 1:
        raise AssertionError("the unit-ball try was not identified: %d candidate blocks %s" % (len(tries), [b["label"] for b in tries]))
    t = tries[0]
    parents = re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", t["note"])
    name = max(parents, key=lambda p: int(p[1]))[0]
    header = ".L" + name
    first = next(i for i, b in enumerate(blocks) if b["label"] == header)
    last = max(i for i, b in enumerate(blocks) if re.search(r"(Header=|Parent Loop )%s\b" % name, b["note"]))
    run = blocks[first:last + 1]
    zeros = [(b["label"], sum(bool(_ZERO_MOVE.match(c)) for c in b["code"])) for b in run]
    return {"try_block": t, "header": header, "blocks": run, "zero_moves": sum(n for _, n in zeros),
            "zero_by_block": [(l, n) for l, n in zeros if n]}


def shade_kernels():
    """{name: (kernel of isa_report.parse, trip_loop of its listing)}: one compile per process."""
    if not _SHADE:
        asm = isa_report.compile_asm(os.path.join(ROOT, "path_tracing_amd", "csrc", "pt_shade.hip"))
        blocks = isa_report.listing(asm)
        for k in isa_report.parse(asm):
            if k["name"].startswith("k_shade<"):
                _SHADE[k["name"]] = (k, trip_loop(blocks[k["name"]]))
    return _SHADE


needs_hipcc = pytest.mark.skipif(isa_report.find_hipcc() is None, reason="hipcc not found: the assembly cannot be produced")


@needs_hipcc
def test_every_instantiation_is_there():
    assert sorted(shade_kernels()) == sorted(PARENT)
    assert PARENT["k_shade<0,0>"][0] - PARENT["k_shade<0,0>"][1] == 153


@needs_hipcc
@pytest.mark.parametrize("name", list(PARENT))
def test_no_zero_fills_at_the_head_of_a_trip(name):
    k, loop = shade_kernels()[name]
    zeros, head = PARENT[name]
    print("%s: %d VALU, trip loop %s of %d blocks: %d zero moves (parent %d, %d of them in the head blocks) %s" % (
        name, k["counts"]["valu"], loop["header"], len(loop["blocks"]), loop["zero_moves"], zeros, head, loop["zero_by_block"]))
    assert k["counts"]["valu"] > 2000 and len(loop["blocks"]) > 100        # the parser saw the kernel and its loop
    assert loop["zero_moves"] <= zeros - head


@needs_hipcc
@pytest.mark.parametrize("name", list(PARENT))
def test_the_unit_ball_try_is_short(name):
    _, loop = shade_kernels()[name]
    code = loop["try_block"]["code"]
    valu = sum(c.startswith("v_") for c in code)
    mads = sum(c.startswith("v_mad_u64_u32") for c in code)
    quarter = mads + sum(c.startswith(("v_mul_lo_u32", "v_mul_hi_u32")) for c in code)
    print("%s: try block %s, %d VALU (parent %d), %d quarter-rate multiplies (parent 10)" % (
        name, loop["try_block"]["label"], valu, PARENT_TRY_VALU, quarter))
    assert mads >= 3 and any(c.startswith("v_cvt_f32_u32") for c in code)  # it is the try: three stream steps, three converts
    assert valu <= PARENT_TRY_VALU - TRY_SAVED


@needs_hipcc
@pytest.mark.parametrize("name", list(PARENT))
def test_registers_cost_no_occupancy_and_nothing_spills(name):
    k, _ = shade_kernels()[name]
    print("%s: %s VGPRs, %d scratch instructions, %s VGPRs spilled, %s SGPRs spilled" % (
        name, k["meta"]["vgpr_count"], k["counts"]["scratch"], k["meta"]["vgpr_spill_count"], k["meta"]["sgpr_spill_count"]))
    assert k["meta"]["vgpr_count"] + k["meta"]["agpr_count"] <= MAX_VGPRS
    assert k["counts"]["scratch"] == 0
    assert k["meta"]["vgpr_spill_count"] == 0


def test_the_trip_loop_is_found_in_a_hand_written_listing():
    """isa_report.listing() and trip_loop() on a hand-written kernel: no compiler needed."""
    asm = "\n".join([
        "\t.globl\t_Z3fooILb0ELb0EEvPf", "_Z3fooILb0ELb0EEvPf:", "; %bb.0:", "\tv_mov_b32_e32 v9, 0",
        ".LBB0_1:                                ; =>This Loop Header: Depth=1",
        "                                        ;     Child Loop BB0_2 Depth 2",
        "\tv_mov_b32_e32 v1, 0", "\tv_mov_b32_e32 v2, 0x3f800000", "\tv_mov_b32_e32 v3, 0 ; a comment",
        ".LBB0_2:                                ;   Parent Loop BB0_1 Depth=1",
        "                                        ; =>  This Inner Loop Header: Depth=2",
        "\tv_mad_u64_u32 v[4:5], s[4:5], v4, s6, v[6:7]", "\tv_mad_u64_u32 v[4:5], s[4:5], v4, s6, v[6:7]",
        "\tv_mad_u64_u32 v[4:5], s[4:5], v4, s6, v[6:7]", "\tv_cvt_f32_u32_e32 v8, v4", "\tv_cvt_f32_u32_e32 v9, v4",
        "\tv_cvt_f32_u32_e32 v10, v4", "\tv_cmp_nle_f32_e32 vcc, 1.0, v8", "\ts_cbranch_execnz .LBB0_2",
        "; %bb.3:                                ;   in Loop: Header=BB0_1 Depth=1", "\tv_mov_b32_e32 v4, 0", "\ts_cbranch_scc1 .LBB0_1",
        "; %bb.4:", "\tv_mov_b32_e32 v5, 0", "\ts_endpgm", ".Lfunc_end0:",
        "amdhsa.kernels:", "  - .agpr_count:     0", "    .name:           _Z3fooILb0ELb0EEvPf", "    .sgpr_count:     12",
        "    .sgpr_spill_count: 0", "    .vgpr_count:     10", "    .vgpr_spill_count: 0", "amdhsa.target:   amdgcn-amd-amdhsa--gfx950"])
    blocks = isa_report.listing(asm)["foo<0,0>"]
    assert [b["label"] for b in blocks] == ["entry", ".LBB0_1", ".LBB0_2", "%bb.3", "%bb.4"]
    loop = trip_loop(blocks)
    assert loop["header"] == ".LBB0_1" and loop["try_block"]["label"] == ".LBB0_2"
    assert [b["label"] for b in loop["blocks"]] == [".LBB0_1", ".LBB0_2", "%bb.3"]
    assert loop["zero_moves"] == 3 and loop["zero_by_block"] == [(".LBB0_1", 2), ("%bb.3", 1)]
    with pytest.raises(AssertionError):
        trip_loop(blocks[:2] + blocks[3:])                        # no block looks like the try: refused, not guessed
