"""A lint over the gfx950 assembly of the library's kernels (tests/test_isa_lint.py drives it).

The compiler's hazard recogniser pads the wait states between instructions it emitted itself and does not look inside an
inline-asm string.  Every SiLU output of this library is written by v_fma_mixlo/hi_f16 inside such strings
(csrc/irmv_common.hpp), and an MFMA that reads such a register fewer than two wait states later reads the register's old
value: no fault, no message, outputs that are wrong on some lanes.  This module reads the compiler's `-S` output and checks
the machine code itself.

Parsing.  A function is the text between `.type NAME,@function` and `.Lfunc_endN:`.  Inside it, lines are labels
(`NAME:`), directives (leading `.`), comments (leading `;`, of which `;;#ASMSTART` / `;;#ASMEND` delimit an inline-asm
region) or instructions: an opcode and comma-separated operands.  Registers are `vN`, `v[a:b]`, `aN`, `a[a:b]`, taken
as sets of (file, index), so a write of v[98:99] meets a read of v99.

Wait states.  `s_nop N` is N + 1 states, any other instruction is one.  The distance of a producer and a consumer is the
number of states strictly between them: adjacent instructions are 0 apart, one `s_nop 0` between them makes 1, one
`s_nop 1` makes 2.

Control flow.  Labels and s_branch / s_cbranch_* give every instruction its set of direct predecessors, so a producer
that ends a block is checked against a consumer that opens each successor.  A branch whose target is no label of its
function, or an indirect jump, raises LintError: the lint cannot vouch for code it cannot follow.

Rules (the pairs of the CDNA3/4 ISA guide's table of required software wait states that can occur around this tree's
asm strings):
  R1  VALU write of a VGPR -> v_mfma_* reading it as A or B: 2 states, on every path, over ALL code.  MFMAs, DS / VMEM
      and SALU instructions are no VALU producers.
  R2  for asm regions that hold an instruction: VGPR written inside -> MFMA A / B / C operand: 2 states;
      -> v_readfirstlane / v_readlane / v_permlane* reading it: 1 state.
  R3  the opcodes found inside asm regions (asm_opcodes) are compared with an allow-list by the test.
  R4  fence_census: per function, the MFMAs whose A / B operand was last written (in program order) inside an asm region,
      and the asm regions that consist of `s_nop 1` (mfma_operand_fence): every such MFMA needs a fence region between
      that write and itself, else its fence has been compiled away, or it never had one (program order, not the
      control-flow graph: see fence_census).
"""
from __future__ import annotations

import re
from collections import namedtuple
from functools import lru_cache

MFMA_NEED = 2        # VALU write -> MFMA SrcA/B/C read
LANE_NEED = 1        # VALU write -> v_readlane / v_readfirstlane / v_permlane* read
WINDOW = 8           # R1's census looks this many states back (violations are the pairs closer than MFMA_NEED)


class LintError(Exception):
    """The assembly cannot be linted (unresolved branch target, malformed text)."""


Insn = namedtuple("Insn", "line op ops asm text")          # asm: id of the enclosing asm region, or -1
Violation = namedtuple("Violation", "rule kernel line producer consumer distance need")

_REG = re.compile(r"(?<![\w.])([va])(?:(\d+)|\[(\d+):(\d+)\])(?!\w)")
_LABEL = re.compile(r"^([.\w$]+):")
_TYPE = re.compile(r"^\s*\.type\s+([.\w$]+),@function")
_FUNC_END = re.compile(r"^\.Lfunc_end\d+:")


@lru_cache(maxsize=None)
def regs(operand: str) -> frozenset:
    out = set()
    for f, n, lo, hi in _REG.findall(operand):
        if n:
            out.add((f, int(n)))
        else:
            out.update((f, i) for i in range(int(lo), int(hi) + 1))
    return frozenset(out)


def split_operands(text: str):
    ops, depth, cur = [], 0, []
    for ch in text:
        if ch in "[(":
            depth += 1
        elif ch in "])":
            depth -= 1
        if ch == "," and depth == 0:
            ops.append("".join(cur).strip())
            cur = []
        else:
            cur.append(ch)
    tail = "".join(cur).strip()
    if tail:
        ops.append(tail)
    return tuple(ops)


def is_mfma(op: str) -> bool:
    return op.startswith("v_mfma_") or op.startswith("v_smfmac_")


def is_lane_reader(op: str) -> bool:
    return op.startswith("v_readfirstlane") or op.startswith("v_readlane") or op.startswith("v_permlane")


def _two_dests(op: str) -> bool:
    return op.startswith("v_swap") or (op.startswith("v_permlane") and "swap" in op)


def _no_dest(op: str) -> bool:
    """Instructions whose first operand is an address or data, not a result."""
    return (op.startswith("s_") or op.startswith("ds_write") or "_store" in op or op.startswith("v_cmp")
            or op.startswith("v_nop") or op.startswith("ds_nop") or op.startswith("buffer_wbl2") or op.startswith("buffer_inv"))


# VALU opcodes whose first operand is no VGPR / AGPR result: the compares (SGPR pair or VCC), the lane reads (an SGPR), v_nop
_VALU_NO_VGPR_DEST = ("v_cmp", "v_readlane", "v_readfirstlane", "v_nop")


def check_shape(i: Insn, where: str):
    """The destination model is: the first operand is the result (the first two for the swaps), except for the opcode
    families of _no_dest.  Today's ISA fits; a `v_` instruction whose first operand holds no VGPR / AGPR and that is not one
    of the known SGPR-result families would be a producer the rules silently miss, so it fails the lint instead."""
    if i.op.startswith("v_") and not i.op.startswith(_VALU_NO_VGPR_DEST) and not (i.ops and regs(i.ops[0])):
        raise LintError(f"{where}: line {i.line}: `{i.text}`: a vector instruction whose first operand is no VGPR / AGPR: "
                        "teach isa_lint.writes its destination")


def writes(i: Insn) -> frozenset:
    """The VGPRs / AGPRs an instruction writes (every kind of instruction: VALU, MFMA, loads)."""
    if not i.ops or _no_dest(i.op):
        return frozenset()
    w = regs(i.ops[0])
    if _two_dests(i.op) and len(i.ops) > 1:
        w = w | regs(i.ops[1])
    return w


def is_valu_producer(i: Insn) -> bool:
    return i.op.startswith("v_") and not is_mfma(i.op)


def states(i: Insn) -> int:
    if i.op == "s_nop":
        return int(i.ops[0], 0) + 1
    return 1


def mfma_ab(i: Insn) -> frozenset:
    return regs(i.ops[1]) | regs(i.ops[2])


def mfma_abc(i: Insn) -> frozenset:
    return mfma_ab(i) | (regs(i.ops[3]) if len(i.ops) > 3 else frozenset())


def lane_reads(i: Insn) -> frozenset:
    srcs = i.ops if _two_dests(i.op) else i.ops[1:]
    r = frozenset()
    for o in srcs:
        r = r | regs(o)
    return r


class Function:
    """One function's instructions with the predecessor relation of its control-flow graph."""

    def __init__(self, name: str, is_kernel: bool = True):
        self.name, self.is_kernel = name, is_kernel
        self.insns = []
        self.labels = {}            # label -> index of the instruction that follows it
        self.extra_preds = {}       # index -> [indices of branches that jump to it]
        self.n_regions = 0

    def finish(self):
        n = len(self.insns)
        for j, i in enumerate(self.insns):
            if i.op in ("s_setpc_b64", "s_swappc_b64") or i.op.startswith("s_call") or "fork" in i.op:
                raise LintError(f"{self.name}: line {i.line}: `{i.text}`: an indirect jump cannot be followed")
            if i.op == "s_branch" or i.op.startswith("s_cbranch_"):
                t = i.ops[0] if i.ops else ""
                if t not in self.labels:
                    raise LintError(f"{self.name}: line {i.line}: `{i.text}`: branch target is no label of this function")
                k = self.labels[t]
                if k < n:
                    self.extra_preds.setdefault(k, []).append(j)

    def preds(self, k: int):
        p = list(self.extra_preds.get(k, ()))
        if k > 0 and self.insns[k - 1].op not in ("s_branch", "s_endpgm"):
            p.append(k - 1)
        return p

    def back(self, k: int, limit: int):
        """(index, distance) of every instruction that can run before instruction k with fewer than `limit` states between."""
        stack = [(p, 0) for p in self.preds(k)]
        seen = set()
        while stack:
            item = stack.pop()
            if item in seen:
                continue
            seen.add(item)
            yield item
            j, d = item
            d2 = d + states(self.insns[j])
            if d2 < limit:
                stack.extend((p, d2) for p in self.preds(j))


def parse(text: str, whole: bool = False):
    """The functions of a `-S` file.  whole=True: a bare snippet (no .type / .Lfunc_end) is one function "snippet"."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+([.\w$]+)", text, re.M))
    funcs, cur, region, pending = [], None, -1, None
    if whole:
        cur = Function("snippet")
    for ln, raw in enumerate(text.splitlines(), 1):
        if cur is None:
            m = _TYPE.match(raw)
            if m:
                pending = m.group(1)
            elif pending is not None and raw.startswith(pending + ":"):
                cur, pending, region = Function(raw.split(":")[0], raw.split(":")[0] in kernels), None, -1
            continue
        if not whole and _FUNC_END.match(raw):
            if region != -1:
                raise LintError(f"{cur.name}: line {ln}: asm region left open")
            cur.finish()
            funcs.append(cur)
            cur = None
            continue
        s = raw.strip()
        if s.startswith(";;#ASMSTART"):
            region = cur.n_regions
            cur.n_regions += 1
            continue
        if s.startswith(";;#ASMEND"):
            region = -1
            continue
        s = s.split(";", 1)[0].strip()
        if not s:
            continue
        m = _LABEL.match(s)
        if m:
            cur.labels[m.group(1)] = len(cur.insns)
            s = s[m.end():].strip()
            if not s:
                continue
        if s.startswith("."):
            continue
        parts = s.split(None, 1)
        cur.insns.append(Insn(ln, parts[0], split_operands(parts[1]) if len(parts) > 1 else (), region, s))
        check_shape(cur.insns[-1], cur.name)
    if whole:
        cur.finish()
        funcs.append(cur)
    elif cur is not None:
        raise LintError(f"{cur.name}: function never ends")
    return funcs


# ---- the rules ---------------------------------------------------------------------------------------------------------
def rule1(funcs):
    """-> (violations, census): census = MFMAs, (VALU producer, MFMA) pairs within WINDOW states, the least distance seen."""
    viol, n_mfma, pairs, dmin = [], 0, 0, None
    for f in funcs:
        for k, c in enumerate(f.insns):
            if not is_mfma(c.op):
                continue
            n_mfma += 1
            need = mfma_ab(c)
            for j, d in f.back(k, WINDOW):
                p = f.insns[j]
                if is_valu_producer(p) and writes(p) & need:
                    pairs += 1
                    dmin = d if dmin is None else min(dmin, d)
                    if d < MFMA_NEED:
                        viol.append(Violation("R1", f.name, c.line, f"{p.line}: {p.text}", c.text, d, MFMA_NEED))
    return viol, {"kernels": len(funcs), "mfmas": n_mfma, "pairs": pairs, "min_distance": dmin}


def rule2(funcs):
    viol = []
    for f in funcs:
        if not any(i.asm >= 0 for i in f.insns):
            continue
        for k, c in enumerate(f.insns):
            if is_mfma(c.op):
                need, lim = mfma_abc(c), MFMA_NEED
            elif is_lane_reader(c.op):
                need, lim = lane_reads(c), LANE_NEED
            else:
                continue
            for j, d in f.back(k, lim):
                p = f.insns[j]
                if p.asm >= 0 and writes(p) & need:
                    viol.append(Violation("R2", f.name, c.line, f"{p.line}: {p.text}", c.text, d, lim))
    return viol


def asm_opcodes(funcs):
    """{opcode: count} over every asm region."""
    out = {}
    for f in funcs:
        for i in f.insns:
            if i.asm >= 0:
                out[i.op] = out.get(i.op, 0) + 1
    return out


def _is_fence(region_texts):
    return [" ".join(x.split()) for x in region_texts] == ["s_nop 1"]


def fence_census(funcs):
    """{function: (asm_fed_mfmas, fence_regions, unfenced_mfmas)}, only functions where any is non-zero.
    asm_fed_mfmas: MFMAs with an A / B register whose last writer sits inside an asm region.  fence_regions: asm regions
    that are exactly `s_nop 1` (mfma_operand_fence).  unfenced_mfmas: asm-fed MFMAs with no fence region between that
    writer and the MFMA -- counted per MFMA, so a function with two fenced sites of which one lost its fence is seen, also
    where the compiler's scheduling happens to keep the pair two states apart.
    LIMIT: "last writer" and "between" are taken in PROGRAM ORDER (one pass over the text), not over the control-flow
    graph: a writer that reaches the MFMA only through a backward branch is not seen as its writer.  All three fenced
    sites of this tree write, fence and consume in one basic block; R1 and R2, which do follow the graph, are the
    check that does not depend on this."""
    out = {}
    for f in funcs:
        region_ops = {}
        for i in f.insns:
            if i.asm >= 0:
                region_ops.setdefault(i.asm, []).append(i.text)
        fence_ids = {k for k, v in region_ops.items() if _is_fence(v)}
        last, fed, unfenced, last_fence = {}, 0, 0, -1
        for k, i in enumerate(f.insns):
            if i.asm in fence_ids:
                last_fence = k
            if is_mfma(i.op):
                writers = [last[r] for r in mfma_ab(i) if last.get(r, -1) >= 0]
                if writers:
                    fed += 1
                    unfenced += last_fence < max(writers)
            for r in writes(i):
                last[r] = k if i.asm >= 0 else -1
        if fed or fence_ids:
            out[f.name] = (fed, len(fence_ids), unfenced)
    return out


def counts(funcs):
    """{function: (instructions, MFMAs)}: what the tie to the built library compares."""
    return {f.name: (len(f.insns), sum(is_mfma(i.op) for i in f.insns)) for f in funcs}


_DIS_SYM = re.compile(r"^([0-9a-f]+) <([^>]+)>:\s*$")
_DIS_INSN = re.compile(r"^\s+([a-z_0-9]+)\b.*//\s*([0-9A-Fa-f]+):")
_SYMTAB = re.compile(r"^([0-9a-f]+)\s+\S+\s+F\s+\S+\s+([0-9a-f]+)\s+(?:\.\w+\s+)?(\S+)\s*$")


def symbol_sizes(symtab: str):
    """{function: size in bytes} of `llvm-objdump -t` output."""
    return {m.group(3): int(m.group(2), 16) for m in map(_SYMTAB.match, symtab.splitlines()) if m}


def disassembly_counts(text: str, sizes):
    """{function: (instructions, MFMAs)} of `llvm-objdump -d` output of a code object.  Only the bytes inside the symbol's
    size count: what follows up to the next function is alignment fill, which the disassembler prints as instructions."""
    out, cur, end = {}, None, 0
    for raw in text.splitlines():
        m = _DIS_SYM.match(raw)
        if m:
            cur = m.group(2) if m.group(2) in sizes else None
            if cur is not None:
                end = int(m.group(1), 16) + sizes[cur]
                out[cur] = [0, 0]
            continue
        m = _DIS_INSN.match(raw)
        if m and cur is not None and int(m.group(2), 16) < end:
            out[cur][0] += 1
            out[cur][1] += is_mfma(m.group(1))
    return {k: tuple(v) for k, v in out.items()}


def format_violations(viol, limit=20):
    lines = [f"{v.rule} {v.kernel} line {v.line}: `{v.producer}` -> `{v.consumer}`: {v.distance} wait state(s), needs {v.need}"
             for v in viol[:limit]]
    if len(viol) > limit:
        lines.append(f"... and {len(viol) - limit} more")
    return "\n".join(lines)
