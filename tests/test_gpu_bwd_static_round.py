"""render_bwd's rounds as straight-line code (csrc/render_bwd.hip): the 16 steps of a round have compile-time step indices --
pixel constants at constant offsets from a base that never moves, constant lane masks, a last step without the second
accumulator set whose switch reads fetch position 0's entry of the NEXT chunk from the other slot -- and the wave's last round
leaves the sequence behind its last step.  What can go wrong is the split between full rounds and the steps of a partial one,
which depends on the list length m alone (a wave runs m + 15 steps), at lengths test_gpu_bwd_round_boundary.py does not reach:

    m       steps    the walk
    2       17       one full round, then a round of exactly one step (leaves behind step 0)
    3       18       a round of two steps (leaves behind step 1: the other parity of the one-ahead pixel constants)
    18, 19  33, 34   the same behind two full rounds, i.e. in the accumulator set and entry slot of the other parity
    34      49       behind three full rounds

* on the device (-m gpu): that file's 40 x 24 image and stack of translucent Gaussians, all five lengths with one image and
  m = 2, 18 in the three other kernel modes; every gradient against the CPU oracle at its TOL = 1e-5 of the tensor maximum,
  every element, and two backwards give equal bits (both inside `_run`);
* in the generated code (no GPU): no instruction of a round body writes the register the pixel constants are addressed with.
"""
import re

import pytest

from test_gpu_bwd_round_boundary import _backward_code_object, _run

LENGTHS = [2, 3, 18, 19, 34]


@pytest.mark.gpu
@pytest.mark.parametrize("m", LENGTHS)
def test_partial_rounds_behind_full_rounds_one_image(oracle, monkeypatch, m):
    _run(oracle, monkeypatch, m, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2, 3], ids=["with-opacity", "second-image-arbitrary-colours", "second-image-colours-one"])
@pytest.mark.parametrize("m", [2, 18])
def test_partial_rounds_behind_full_rounds_other_kernel_modes(oracle, monkeypatch, m, mode):
    _run(oracle, monkeypatch, m, mode)


# ---------------------------------------------------------------------------------------------------------------
# generated code
# ---------------------------------------------------------------------------------------------------------------
_PIXEL_READ = re.compile(r"^ds_read(?:2|2st64)?_b64 v\[\d+:\d+\], v(\d+)\b")  # the pixel constants are float2 pairs
_SWITCH_READ = re.compile(r"^ds_read_b128 v\[\d+:\d+\], v\d+(?: offset:(\d+))?$")
_ROUND_START = ("global_", "ds_write", "s_endpgm")  # gathers, stores and staging: what a round start has and a step has not


def _round_bodies(code):
    """The round bodies of one kernel.  HOW A BODY IS LOCATED: the instruction stream is cut at every instruction only a
    round start (or the prologue / epilogue) has -- a global load or store, an LDS write, the end of the program; a piece
    that holds 16 entry-switch statements (each begins with the first `ds_read_b128` of a group of reads) is the 16 steps of
    a round, from behind the round start's last memory instruction to the last step's wait."""
    pieces, cur = [], []
    for ins in code:
        if ins.startswith(_ROUND_START):
            pieces.append(cur)
            cur = []
        else:
            cur.append(ins)
    pieces.append(cur)
    bodies = []
    for p in pieces:
        switches = [i for i, ins in enumerate(p) if _SWITCH_READ.match(ins) and not (i and _SWITCH_READ.match(p[i - 1]))]
        if len(switches) == 16:
            bodies.append((p, switches))
    return bodies


def test_no_instruction_of_a_round_body_advances_the_pixel_constant_address():
    """In each of the four kernels: two round bodies (one per accumulator-set parity).  In a body the pixel constants of the
    steps are read through ONE address register (mode 2: those of the first image), at least 15 reads (steps 0 .. 14 read the next step's; `ds_read2` may pair
    two arrays in one instruction), each at immediate offsets of its own, and no instruction of the body has that register
    as its destination.  The last step's switch reads take from the other slot than the 15 before them."""
    code, _ = _backward_code_object()
    kernels = [k for k in code if "render_bwd_kernel" in k]
    assert len(kernels) == 4, kernels
    for k in kernels:
        bodies = _round_bodies(code[k])
        assert len(bodies) == 2, (k, len(bodies))
        last_slots = []
        for body, switches in bodies:
            reads = [(ins, _PIXEL_READ.match(ins)) for ins in body]
            reads = [(ins, m.group(1)) for ins, m in reads if m]
            regs = [r for _, r in reads]
            reg = max(set(regs), key=regs.count)  # the base: what the reads of the first arrays go through
            if "ILi2E" not in k:
                assert set(regs) == {reg}, (k, set(regs))
            else:  # (the compiler reaches the second image's two arrays, beyond the range of an immediate, through a
                   # temporary = base + constant per step; the base itself must stay what it is all the same)
                assert regs.count(reg) >= 15, (k, regs)
            # no two reads take from the same place: the steps differ by the immediate offsets alone
            based = [re.sub(r"v\[\d+:\d+\]", "", ins) for ins, r in reads if r == reg]
            assert len(based) >= 15 and len(set(based)) == len(based), (k, based)
            written = [ins for ins in body if re.match(r"^\S+\s+v%s\b" % reg, ins) or re.match(r"^\S+\s+v\[%s:" % reg, ins)]
            assert not written, (k, written)
            slot = [int(_SWITCH_READ.match(body[i]).group(1) or 0) for i in switches]
            assert len(set(slot[:15])) == 1 and slot[15] != slot[0], (k, slot)
            last_slots.append(slot[15])
            print(k[:28], "address register v%s," % reg, len(reads), "pixel-constant reads, switch slots", slot[0], "->", slot[15])
        assert last_slots[0] != last_slots[1], (k, last_slots)  # the two parities read ahead from opposite slots
