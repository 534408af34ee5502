"""The compiled gfx950 ISA of every kernel source, linted for the hazards the compiler does not pad (tests/isa_lint.py: the
parser, the wait-state model and rules R1 - R4), and tied to the library that runs.

  * the ISA under test: every entry of _build.SOURCES with device code, compiled with exactly _build.COMMON + its extra
    flags + IRMV_EXTRA_HIPCC_FLAGS, plus `--cuda-device-only -S`, into a tmp directory (kept under the pytest cache
    directory, keyed by _build.source_hash(), the extra flags and the compiler's version: k_conv.hip alone takes two
    minutes);
  * the tie: the gfx950 code objects inside the built libirmv_hip.so, disassembled, have per function the same number of
    instructions and of MFMAs as that text;
  * R1 - R4 hold on the committed tree (the census is printed);
  * red controls: with both mfma_operand_fence bodies emptied (on a tmp copy of csrc/) R1, R2 and R4 fail in k_kpt.hip and
    k_conv.hip; hand-written snippets show each thing the parser must see (a producer in the predecessor block, s_nop
    counting, register ranges, destinations that are no operands).
"""
import hashlib
import os
import re
import shutil
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

import isa_lint
from irmv_detection_amd import _build

JOBS = 16
# R3: the opcodes inline asm may hold today.  A new one has hazards of its own: look its pairs up in the ISA guide's table
# of required software wait states ("Manually Inserted Wait States"), extend isa_lint.rule2 where one can occur at an asm
# boundary, and only then add the opcode here.
ASM_OPCODES = {"v_fma_mixlo_f16", "v_fma_mixhi_f16", "v_pk_max_f16", "s_nop"}
FENCED = ("k_kpt.hip", "k_conv.hip")     # the sources with mfma_operand_fence call sites
FENCE_BODY = re.compile(r'asm volatile\("s_nop 1"[^;]*;')


def _extra_flags():
    return os.environ.get("IRMV_EXTRA_HIPCC_FLAGS", "").split()


def _device_sources():
    return [(s, x) for s, x in _build.SOURCES if "__global__" in open(os.path.join(_build.CSRC, s)).read()]


def _llvm_tool(name):
    cc = os.path.realpath(_build.hipcc())
    root = os.path.dirname(os.path.dirname(cc))
    for cand in (os.path.join(root, "lib", "llvm", "bin", name), os.path.join(root, "llvm", "bin", name), shutil.which(name)):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError(f"{name} not found next to {cc}")


def _compile(job):
    src_dir, src, extra, out = job
    cmd = [_build.hipcc()] + _build.COMMON + extra + _extra_flags() + ["--cuda-device-only", "-S", os.path.join(src_dir, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr[-4000:]}"
    return out


@pytest.fixture(scope="module")
def isa(tmp_path_factory, request):
    """{"tree": {source: assembly text}, "nofence": {source: assembly text of FENCED with the fence bodies emptied}}."""
    t0 = time.time()
    version = subprocess.run([_build.hipcc(), "--version"], capture_output=True, text=True).stdout
    key = hashlib.sha256((_build.source_hash() + "\0" + " ".join(_extra_flags()) + "\0" + version).encode()).hexdigest()[:24]
    cache = getattr(request.config, "cache", None)
    keep = os.path.join(str(cache.mkdir("isa_lint")), key) if cache is not None else None
    work = str(tmp_path_factory.mktemp("isa"))
    nofence_src = os.path.join(work, "csrc")
    shutil.copytree(_build.CSRC, nofence_src)
    hdr = os.path.join(nofence_src, "irmv_common.hpp")
    text, n = FENCE_BODY.subn("", open(hdr).read())
    assert n == 2, "mfma_operand_fence: expected two overloads with an `s_nop 1` body"
    open(hdr, "w").write(text)
    emptied = hashlib.sha256(text.encode()).hexdigest()[:12]     # the red control's files are keyed by what the emptying produced
    want = {("tree", s): (_build.CSRC, s, x) for s, x in _device_sources()}
    want.update({("nofence", s): (nofence_src, s, dict(_build.SOURCES)[s]) for s in FENCED})
    paths, jobs = {}, []
    for (kind, s), (d, _, x) in want.items():
        name = f"{kind}{'-' + emptied if kind == 'nofence' else ''}_{os.path.splitext(s)[0]}.s"
        if keep and os.path.exists(os.path.join(keep, name)):
            paths[(kind, s)] = os.path.join(keep, name)
        else:
            paths[(kind, s)] = os.path.join(work, name)
            jobs.append((d, s, x, paths[(kind, s)]))
    with ThreadPoolExecutor(max_workers=min(JOBS, max(1, len(jobs)))) as pool:
        list(pool.map(_compile, jobs))
    if keep and jobs:
        os.makedirs(keep, exist_ok=True)
        for _, _, _, out in jobs:
            shutil.copyfile(out, os.path.join(keep, os.path.basename(out)) + ".part")
            os.replace(os.path.join(keep, os.path.basename(out)) + ".part", os.path.join(keep, os.path.basename(out)))
    out = {"tree": {}, "nofence": {}}
    for (kind, s), p in paths.items():
        out[kind][s] = isa_lint.parse(open(p).read())
    print(f"\n[isa lint] {len(jobs)} of {len(want)} sources compiled, the rest from the cache; compiled and parsed in {time.time() - t0:.1f} s")
    return out


# ---- the tie to the library ------------------------------------------------------------------------------------------------
def test_the_linted_text_is_the_code_of_the_built_library(isa, tmp_path, capsys):
    """Every function of every code object in libirmv_hip.so has the instruction and MFMA counts of the `-S` text, and
    the other way round."""
    lib = _build.build()
    fat = tmp_path / "fatbin"
    subprocess.check_call([_llvm_tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, str(tmp_path / "discard")])
    data = fat.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(magic, data)]
    assert starts, "no offload bundle in .hip_fatbin (a compressed bundle would need unbundling first)"
    in_lib = {}
    for i, a in enumerate(starts):
        b = tmp_path / f"bundle{i}"
        b.write_bytes(data[a:starts[i + 1] if i + 1 < len(starts) else len(data)])
        co = tmp_path / f"bundle{i}.co"
        subprocess.check_call([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={b}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        if co.stat().st_size == 0:
            continue
        dis = subprocess.run([_llvm_tool("llvm-objdump"), "-d", str(co)], capture_output=True, text=True, check=True).stdout
        symtab = subprocess.run([_llvm_tool("llvm-objdump"), "-t", str(co)], capture_output=True, text=True, check=True).stdout
        for sym, c in isa_lint.disassembly_counts(dis, isa_lint.symbol_sizes(symtab)).items():
            in_lib.setdefault(sym, []).append(c)
    in_text = {}
    for src, funcs in isa["tree"].items():
        for name, c in isa_lint.counts(funcs).items():
            in_text.setdefault(name, []).append((src, c))
    differ = [f"{name}: {src} has (instructions, MFMAs) {c}, the library {in_lib.get(name)}"
              for name, v in in_text.items() for src, c in v if c not in in_lib.get(name, [])]
    missing = sorted(set(in_lib) - set(in_text))
    with capsys.disabled():
        print(f"\n[isa lint] tie: {len(in_text)} functions of {len(isa['tree'])} sources, {sum(c[0] for v in in_text.values() for _, c in v)} "
              f"instructions, {sum(c[1] for v in in_text.values() for _, c in v)} MFMAs; the library holds {len(starts)} bundles with "
              f"{len(in_lib)} functions; {len(differ)} differ, {len(missing)} only in the library")
    assert not differ, "\n".join(differ[:20])
    assert not missing, missing[:20]


# ---- the committed tree ----------------------------------------------------------------------------------------------------
def test_r1_r2_no_valu_write_reaches_an_mfma_or_lane_read_too_early(isa, capsys):
    bad, lines = [], []
    for src, funcs in isa["tree"].items():
        v1, census = isa_lint.rule1(funcs)
        v2 = isa_lint.rule2(funcs)
        bad += v1 + v2
        lines.append(f"[isa lint] {src:14s} kernels {census['kernels']:4d}  MFMAs {census['mfmas']:6d}  pairs examined {census['pairs']:5d}  "
                     f"min distance {census['min_distance']}  R1 {len(v1)}  R2 {len(v2)}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, isa_lint.format_violations(bad)


def test_r3_asm_opcodes_are_the_allow_list(isa, capsys):
    seen = {}
    for src, funcs in isa["tree"].items():
        for op, n in isa_lint.asm_opcodes(funcs).items():
            seen[op] = seen.get(op, 0) + n
    with capsys.disabled():
        print(f"\n[isa lint] opcodes inside asm regions: {dict(sorted(seen.items()))}")
    assert set(seen) == ASM_OPCODES, (f"asm regions hold {sorted(set(seen) ^ ASM_OPCODES)} beside / short of the allow-list: look the new opcode's pairs up in the "
                                      "ISA guide's table of required software wait states, extend isa_lint.rule2 for those that can "
                                      "occur at an asm boundary, then extend ASM_OPCODES in this file")


def _call_sites(src):
    return len(re.findall(r"\bmfma_operand_fence\s*\(", open(os.path.join(_build.CSRC, src)).read()))


def test_r4_every_fence_call_site_is_in_the_isa(isa, capsys):
    """Every MFMA that reads what inline asm wrote last has an `s_nop 1` region between that write and itself (counted per
    MFMA: one lost fence of two in a function is seen); sources with call sites have at least as many fenced functions as
    call sites and no fence region in a function without an asm-fed MFMA; sources without call sites have no asm-fed MFMA
    at all (one would need a fence).  isa_lint.fence_census states the limit: program order, not the control-flow graph."""
    lines = []
    for src, funcs in isa["tree"].items():
        sites, census = _call_sites(src), isa_lint.fence_census(funcs)
        fed = {k: v for k, v in census.items() if v[0]}
        unfenced = sorted(k for k, v in fed.items() if v[2])
        lines.append(f"[isa lint] {src:14s} fence call sites {sites}, functions with asm-fed MFMAs {len(fed)} ({sum(v[0] for v in fed.values())} MFMAs, "
                     f"{sum(v[2] for v in fed.values())} unfenced), `s_nop 1` regions {sum(v[1] for v in census.values())}")
        assert (src in FENCED) == (sites > 0), src
        assert not unfenced, (src, "an MFMA reads what inline asm wrote and no mfma_operand_fence lies between, in", unfenced[:5])
        assert len(fed) >= sites, (src, "fewer fenced instantiations than call sites")
        assert all(v[0] for v in census.values()), (src, "an `s_nop 1` region in a function without an asm-fed MFMA")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ---- red controls -----------------------------------------------------------------------------------------------------------
def test_red_emptied_fences_are_reported(isa, capsys):
    """Both mfma_operand_fence bodies emptied: on today's tree 9 violations in k_kpt.hip (three per kpt3_kernel
    instantiation) and 17 in k_conv.hip -- 15 at the keypoint final of conv_mfma_kernel / conv_mfma_multi, 2 at the fused
    Detect final of one conv3x3_lds_kernel instantiation; the other instantiations of that site are two states apart by
    the compiler's scheduling alone.  R4 reports every one of them."""
    lines = []
    for src in FENCED:
        funcs = isa["nofence"][src]
        v1, _ = isa_lint.rule1(funcs)
        v2 = isa_lint.rule2(funcs)
        census = isa_lint.fence_census(funcs)
        unfenced = [k for k, v in census.items() if v[2]]
        lines.append(f"[isa lint] red, fences emptied: {src}: R1 {len(v1)}, R2 {len(v2)} in {len({v.kernel for v in v1 + v2})} functions; "
                     f"R4: {len(unfenced)} functions with asm-fed MFMAs and no fence\n" + isa_lint.format_violations(v1, 3))
        assert len(v1) >= 1 and len(v2) >= 1, src
        assert all(v.distance < isa_lint.MFMA_NEED and "v_fma_mix" in v.producer and isa_lint.is_mfma(v.consumer.split()[0]) for v in v1 + v2)
        assert {(v.kernel, v.line) for v in v1} <= {(v.kernel, v.line) for v in v2}    # R1's pairs here have their producer in asm: R2 sees them too
        assert unfenced and sum(v[1] for v in census.values()) == 0
        assert len(unfenced) == len([k for k, v in isa_lint.fence_census(isa["tree"][src]).items() if v[0]])
        assert all(v[2] == v[0] for v in census.values())       # every asm-fed MFMA is reported, the safe-by-luck ones too
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    kpt = isa_lint.rule1(isa["nofence"]["k_kpt.hip"])[0]
    assert len({v.kernel for v in kpt}) == 3      # every kpt3_kernel instantiation


def _lint(snippet):
    funcs = isa_lint.parse(snippet, whole=True)
    return isa_lint.rule1(funcs)[0], isa_lint.rule2(funcs)


MFMA = "v_mfma_f32_16x16x16_f16 v[94:97], v[116:117], v[98:99], 0"
SNIPPETS = [
    # (id, text, R1 violations, R2 violations, distance reported)
    ("producer in the predecessor block, MFMA first in the branch target",
     f";;#ASMSTART\nv_fma_mixhi_f16 v99, v97, v101, 0\n;;#ASMEND\ns_cbranch_scc1 .LBB0_2\ns_nop 7\n.LBB0_1:\ns_nop 7\n.LBB0_2:\n{MFMA}\n", 1, 1, 1),
    ("adjacent",
     f";;#ASMSTART\nv_fma_mixhi_f16 v99, v97, v101, 0\n;;#ASMEND\n{MFMA}\n", 1, 1, 0),
    ("s_nop 0 between producer and MFMA",
     f";;#ASMSTART\nv_fma_mixhi_f16 v99, v97, v101, 0\n;;#ASMEND\ns_nop 0\n{MFMA}\n", 1, 1, 1),
    ("s_nop 1 between them",
     f";;#ASMSTART\nv_fma_mixhi_f16 v99, v97, v101, 0\n;;#ASMEND\n;;#ASMSTART\ns_nop 1\n;;#ASMEND\n{MFMA}\n", 0, 0, None),
    ("two s_nop 0 make two states",
     f";;#ASMSTART\nv_fma_mixhi_f16 v99, v97, v101, 0\n;;#ASMEND\ns_nop 0\ns_nop 0\n{MFMA}\n", 0, 0, None),
    ("write to v[98:99] read as v99",
     "v_pk_max_f16 v[98:99], v[2:3], v[4:5]\nv_mfma_f32_16x16x16_f16 v[94:97], v[116:117], v99, 0\n", 1, 0, 0),
    ("write to a register the MFMA uses only as its destination",
     f";;#ASMSTART\nv_fma_mixhi_f16 v95, v97, v101, 0\n;;#ASMEND\n{MFMA}\n", 0, 0, None),
    ("the C operand is R2's alone",
     ";;#ASMSTART\nv_fma_mixlo_f16 v5, v97, v101, 0\n;;#ASMEND\nv_mfma_f32_16x16x16_f16 v[94:97], v[116:117], v[98:99], v[4:7]\n", 0, 1, 0),
    ("outside asm the producer is R1's alone",
     f"v_fma_mixhi_f16 v99, v97, v101, 0\ns_nop 0\n{MFMA}\n", 1, 0, 1),
    ("an MFMA is no VALU producer",
     f"v_mfma_f32_16x16x16_f16 v[98:101], v[116:117], v[2:3], 0\n{MFMA}\n", 0, 0, None),
    ("the fall-through of an unconditional branch is no path",
     f";;#ASMSTART\nv_fma_mixhi_f16 v99, v97, v101, 0\n;;#ASMEND\ns_branch .LBB0_3\n.LBB0_2:\n{MFMA}\n.LBB0_3:\ns_nop 0\n", 0, 0, None),
]


@pytest.mark.parametrize("tag,text,r1,r2,dist", SNIPPETS, ids=[s[0] for s in SNIPPETS])
def test_snippets(tag, text, r1, r2, dist):
    v1, v2 = _lint(text)
    assert (len(v1), len(v2)) == (r1, r2), isa_lint.format_violations(v1 + v2)
    assert all(v.distance == dist for v in v1 + v2)


def test_snippet_lane_reads_need_one_state():
    bad = ";;#ASMSTART\nv_fma_mixlo_f16 v7, v1, v2, 0\n;;#ASMEND\nv_readfirstlane_b32 s4, v7\n"
    good = ";;#ASMSTART\nv_fma_mixlo_f16 v7, v1, v2, 0\n;;#ASMEND\ns_nop 0\nv_readlane_b32 s4, v7, 3\n"
    assert [len(x) for x in _lint(bad)] == [0, 1] and [len(x) for x in _lint(good)] == [0, 0]
    assert [len(x) for x in _lint(bad.replace("v_readfirstlane_b32 s4, v7", "v_permlane32_swap v7, v9"))] == [0, 1]


def test_snippet_unresolved_branch_target_fails_the_lint():
    with pytest.raises(isa_lint.LintError):
        isa_lint.parse(f"s_cbranch_scc1 .LBB9_9\n{MFMA}\n", whole=True)
    with pytest.raises(isa_lint.LintError):
        isa_lint.parse(f"s_setpc_b64 s[4:5]\n{MFMA}\n", whole=True)


def test_snippet_r4_sees_one_lost_fence_of_two_that_is_safe_by_luck():
    """Two fenced sites in one function; the second lost its fence and sits two states from its MFMA by two `s_nop 0`
    (R1 and R2 are silent): R4 counts it."""
    site = ";;#ASMSTART\nv_fma_mixhi_f16 v99, v97, v101, 0\n;;#ASMEND\n"
    fence = ";;#ASMSTART\ns_nop 1\n;;#ASMEND\n"
    both = isa_lint.parse(site + fence + MFMA + "\n" + site + fence + MFMA + "\n", whole=True)
    lost = isa_lint.parse(site + fence + MFMA + "\n" + site + "s_nop 0\ns_nop 0\n" + MFMA + "\n", whole=True)
    assert isa_lint.fence_census(both)["snippet"] == (2, 2, 0)
    assert isa_lint.fence_census(lost)["snippet"] == (2, 1, 1)
    assert not isa_lint.rule1(lost)[0] and not isa_lint.rule2(lost)


def test_snippet_unknown_destination_shape_fails_the_lint():
    with pytest.raises(isa_lint.LintError):
        isa_lint.parse("v_fma_mixlo_f16 s[4:5], v1, v2, 0\n", whole=True)
    isa_lint.parse("v_readfirstlane_b32 s4, v7\nv_cmp_eq_u32_e32 vcc, v1, v2\n", whole=True)
