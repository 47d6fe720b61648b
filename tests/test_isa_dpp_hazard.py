"""Static check of the compiled gfx950 ISA: no DPP instruction may read a VGPR that a packed-FP32 (v_pk_*) VALU instruction wrote
fewer than 5 wait states earlier.

Why: cm_ffn_fused once computed different bits from run to run.  The compiler packed two tokens' LayerNorm sums into
v_pk_fma_f32 / v_pk_add_f32 and read the high half of the pair by DPP two wait states later (the hazard recognizer's plain
VALU -> DPP distance); lanes 48-63 then saw a stale value left by an earlier workgroup.  The settled helpers in cm_common.h pin
every DPP source behind s_nop 4 (5 wait states), which is the distance this check demands.

The check compiles every csrc/*.hip with the Makefile's flags to assembly (--cuda-device-only -S) and runs a forward dataflow
over each function's control-flow graph: a label joins all of its predecessors and keeps, per VGPR, the SHORTEST distance to a
packed write on any of them, so a branch or loop back-edge never resets the window.  A wait state is one instruction, or N+1
for s_nop N.  Every VGPR a DPP instruction reads counts (the cross-lane source and any other), each half of a pair included.
"""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mamba_asr_amd", "csrc")
MIN_WAIT_STATES = 5

# Sites allowed to stay below MIN_WAIT_STATES, one entry per (function substring, DPP instruction substring), each with its
# reason and the GPU test that runs it past residency.  Empty: every site is padded.
ALLOWLIST = {}


def _hipcc():
    cand = os.environ.get("HIPCC") or shutil.which("hipcc")
    if not cand:
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        cand = os.path.join(rocm, "bin", "hipcc")
    return cand if os.path.isfile(cand) and os.access(cand, os.X_OK) else None


def _makefile_flags():
    """CXXFLAGS of csrc/Makefile with $(ARCH) = gfx950, so the check sees the code the library is built from."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        m = re.search(r"^CXXFLAGS\s*=\s*(.*)$", f.read(), re.M)
    assert m, "csrc/Makefile has no CXXFLAGS line"
    return m.group(1).replace("$(ARCH)", "gfx950").split()


# ---------------------------------------------------------------------------------------------------------------- the analysis

_DPP_CTRL = re.compile(r"\b(quad_perm:|row_shl:|row_shr:|row_ror:|row_mirror\b|row_half_mirror\b|row_bcast|row_newbcast:|"
                       r"row_share:|row_xmask:|wave_shl|wave_shr|wave_rol|wave_ror)")
_VREG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_NOP = re.compile(r"^s_nop\s+(0x[0-9a-fA-F]+|\d+)")


def _vregs(text):
    out = []
    for m in _VREG.finditer(text):
        if m.group(1) is not None:
            out.append(int(m.group(1)))
        else:
            out.extend(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def _operands(rest):
    """Split the operand field at top-level commas (v[4:5] and quad_perm:[1,0,3,2] keep theirs)."""
    ops, depth, cur = [], 0, ""
    for ch in rest:
        if ch == "[":
            depth += 1
        elif ch == "]":
            depth -= 1
        if ch == "," and depth == 0:
            ops.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        ops.append(cur.strip())
    return [op.split(" ", 1)[0] for op in ops]          # the last one carries the modifiers (row_mirror, row_mask:0xf, ...)


class Insn:
    __slots__ = ("text", "mnem", "ops", "line")

    def __init__(self, text, line):
        self.text, self.line = text, line
        head, _, rest = text.partition(" ")
        self.mnem = head
        self.ops = _operands(rest.strip())

    @property
    def wait_states(self):
        m = _NOP.match(self.text)
        return int(m.group(1), 0) + 1 if m else 1

    @property
    def is_dpp(self):
        return self.mnem.endswith("_dpp") or bool(_DPP_CTRL.search(self.text))

    @property
    def is_packed(self):
        return self.mnem.startswith("v_pk_")

    def dst_vregs(self):
        """VGPRs this instruction is known to overwrite (VALU: the first operand).  Anything else writes nothing here, which only
        makes the check stricter: a packed write is forgotten only when a known VALU write replaces it."""
        if not self.mnem.startswith("v_") or not self.ops:
            return []
        if self.is_dpp or self.mnem.startswith("v_writelane") or "PRESERVE" in self.text or "op_sel" in self.text:
            return [] if not self.is_packed else _vregs(self.ops[0])          # may keep some lanes or half of the old value
        return _vregs(self.ops[0])

    def src_vregs(self):
        return [r for op in self.ops[1:] for r in _vregs(op)]


def parse_functions(asm):
    """Assembly text -> {function name: [items]}, an item being ('label', name) or ('insn', Insn)."""
    funcs, cur, name = {}, None, None
    for ln, raw in enumerate(asm.splitlines(), 1):
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = _LABEL.match(line)
        if m:
            lab = m.group(1)
            if lab.startswith(".Lfunc_end"):
                cur, name = None, None
            elif not lab.startswith("."):
                name, cur = lab, []
                funcs[name] = cur
            elif cur is not None:
                cur.append(("label", lab))
            continue
        if cur is None:
            continue
        s = line.strip()
        if s.startswith(".") or not re.match(r"^[a-z]", s):
            continue                                   # directive
        cur.append(("insn", Insn(re.sub(r"\s+", " ", s), ln)))
    return {k: v for k, v in funcs.items() if any(t == "insn" for t, _ in v)}


_UNCOND = ("s_branch",)
_ENDS = ("s_endpgm", "s_setpc_b64", "s_trap")


def _blocks(items):
    """items -> list of (label or None, [Insn]), and successor lists by block index."""
    blocks, labels = [], {}
    cur_lab, cur = None, []

    def close():
        blocks.append((cur_lab, cur))

    for kind, v in items:
        if kind == "label":
            if cur or cur_lab is not None or not blocks:
                close()
            cur_lab, cur = v, []
            labels[v] = len(blocks)
            continue
        cur.append(v)
        if v.mnem.startswith("s_cbranch") or v.mnem in _UNCOND or v.mnem in _ENDS:
            close()
            cur_lab, cur = None, []
    close()
    succ = []
    for i, (_, insns) in enumerate(blocks):
        s = []
        last = insns[-1] if insns else None
        if last is not None and (last.mnem.startswith("s_cbranch") or last.mnem in _UNCOND):
            tgt = last.ops[0] if last.ops else None
            if tgt in labels:
                s.append(labels[tgt])
            else:                                      # unknown target: it could be anywhere; join every block
                s.extend(range(len(blocks)))
        if last is None or not (last.mnem in _UNCOND or last.mnem in _ENDS):
            if i + 1 < len(blocks):
                s.append(i + 1)
        succ.append(s)
    return blocks, succ


def _step(state, insn, report):
    """One instruction over state {vgpr: (wait states since its packed write, the packed Insn)}."""
    if insn.is_dpp:
        for r in sorted(set(insn.src_vregs())):
            if r in state:
                report(r, state[r], insn)
    ws = insn.wait_states
    nxt = {r: (d + ws, p) for r, (d, p) in state.items() if d + ws < MIN_WAIT_STATES}
    for r in insn.dst_vregs():
        nxt.pop(r, None)
    if insn.is_packed:
        for r in insn.dst_vregs():
            nxt[r] = (0, insn)
    return nxt


def _join(states):
    out = {}
    for st in states:
        for r, (d, p) in st.items():
            if r not in out or d < out[r][0]:
                out[r] = (d, p)
    return out


def check_function(name, items):
    """Findings in one function: list of dicts (function, producer, dpp, vgpr, wait_states, line numbers)."""
    blocks, succ = _blocks(items)
    preds = [[] for _ in blocks]
    for i, s in enumerate(succ):
        for j in s:
            preds[j].append(i)
    outs = [None] * len(blocks)
    work = list(range(len(blocks)))
    while work:
        i = work.pop(0)
        st = _join([outs[p] for p in preds[i] if outs[p] is not None])
        for insn in blocks[i][1]:
            st = _step(st, insn, lambda *a: None)
        if st != outs[i]:
            outs[i] = st
            work.extend(j for j in succ[i] if j not in work)
    found = {}

    def report(r, dp, dpp):
        d, prod = dp
        key = (dpp.line, prod.line)
        f = found.setdefault(key, dict(function=name, producer=prod.text, producer_line=prod.line, dpp=dpp.text,
                                       dpp_line=dpp.line, vgprs=[], wait_states=d))
        f["vgprs"].append(r)
        f["wait_states"] = min(f["wait_states"], d)

    for i, (_, insns) in enumerate(blocks):
        st = _join([outs[p] for p in preds[i] if outs[p] is not None])
        for insn in insns:
            st = _step(st, insn, report)
    return sorted(found.values(), key=lambda f: f["dpp_line"])


def check_asm(asm):
    """-> (findings, number of DPP instructions seen)"""
    findings, ndpp = [], 0
    for name, items in parse_functions(asm).items():
        ndpp += sum(1 for k, v in items if k == "insn" and v.is_dpp)
        findings.extend(check_function(name, items))
    return findings, ndpp


def _allowed(f):
    return any(fn in f["function"] and dpp in f["dpp"] for fn, dpp in ALLOWLIST)


def _fmt(f):
    return (f"{f['function']}: '{f['producer']}' (line {f['producer_line']}) -> '{f['dpp']}' (line {f['dpp_line']}) "
            f"reads v{f['vgprs']} after {f['wait_states']} wait state(s) (need {MIN_WAIT_STATES})")


# ------------------------------------------------------------------------------------------------------- negative controls

_KERNEL = "k:\n{}\n.Lfunc_end0:\n"


def _listing(*lines):
    return _KERNEL.format("\n".join(ln if ln.endswith(":") else "\t" + ln for ln in lines))


def test_flags_high_half_read_two_states_after_packed_write():
    # the cm_ffn_fused signature of the pre-fix tree
    asm = _listing("v_pk_add_f32 v[26:27], v[26:27], v[28:29]",
                   "s_nop 1",
                   "v_mov_b32_dpp v29, v27 row_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1",
                   "s_endpgm")
    findings, ndpp = check_asm(asm)
    assert ndpp == 1
    assert len(findings) == 1 and findings[0]["vgprs"] == [27] and findings[0]["wait_states"] == 2, findings
    assert findings[0]["function"] == "k" and "v_pk_add_f32" in findings[0]["producer"] and "_dpp" in findings[0]["dpp"]


def test_flags_low_half_and_fused_dpp_add():
    asm = _listing("v_pk_fma_f32 v[4:5], v[0:1], v[2:3], v[4:5]",
                   "v_mov_b32_e32 v9, v8",
                   "s_nop 2",
                   "v_add_f32_dpp v4, v4, v4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1",
                   "s_endpgm")
    findings, _ = check_asm(asm)
    assert len(findings) == 1 and findings[0]["wait_states"] == 4, findings


def test_passes_behind_s_nop_4():
    asm = _listing("v_pk_add_f32 v[26:27], v[26:27], v[28:29]",
                   "s_nop 4",
                   "v_mov_b32_dpp v29, v27 row_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1",
                   "s_endpgm")
    assert check_asm(asm) == ([], 1)


def test_passes_non_packed_producer():
    asm = _listing("v_add_f32_e32 v27, v26, v27",
                   "v_mov_b32_dpp v29, v27 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1",
                   "s_endpgm")
    assert check_asm(asm) == ([], 1)


def test_overwrite_by_plain_valu_clears_the_packed_write():
    asm = _listing("v_pk_mul_f32 v[2:3], v[2:3], v[4:5]",
                   "v_mov_b32_e32 v3, v7",
                   "v_mov_b32_dpp v8, v3 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1",
                   "s_endpgm")
    assert check_asm(asm) == ([], 1)


def test_window_survives_branches_and_back_edges():
    # a packed write at the end of a loop body reaches the DPP at the loop head over the back-edge; the fall-through block
    # and the label each count, so neither resets the window
    loop = _listing("s_mov_b32 s0, 0",
                    ".LBB0_1:",
                    "v_mov_b32_dpp v10, v3 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1",
                    "v_add_f32_e32 v11, v10, v11",
                    "v_pk_add_f32 v[2:3], v[2:3], v[4:5]",
                    "s_cbranch_scc1 .LBB0_1",
                    "s_endpgm")
    findings, _ = check_asm(loop)
    assert len(findings) == 1 and findings[0]["wait_states"] == 1, findings
    join = _listing("s_cbranch_vccz .LBB0_2",
                    "v_pk_add_f32 v[2:3], v[2:3], v[4:5]",
                    "s_nop 4",
                    "s_branch .LBB0_3",
                    ".LBB0_2:",
                    "v_pk_add_f32 v[2:3], v[2:3], v[4:5]",
                    ".LBB0_3:",
                    "s_nop 1",
                    "v_mov_b32_dpp v10, v2 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1",
                    "s_endpgm")
    findings, _ = check_asm(join)
    assert len(findings) == 1 and findings[0]["wait_states"] == 2, findings   # the short path decides


def test_inline_asm_lines_count():
    # an asm statement's body is instructions like any other (scan_rows_bwd's fused DPP adds live in one)
    asm = _listing("v_pk_add_f32 v[0:1], v[0:1], v[2:3]",
                   ";;#ASMSTART",
                   "s_nop 0",
                   "v_add_f32_dpp v1, v1, v1 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1",
                   ";;#ASMEND",
                   "s_endpgm")
    findings, _ = check_asm(asm)
    assert len(findings) == 1 and findings[0]["wait_states"] == 1, findings


# ------------------------------------------------------------------------------------------------------------ the library

@pytest.fixture(scope="module")
def library_asm(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found (HIPCC, PATH, ROCM_PATH/bin): cannot compile csrc/*.hip to gfx950 assembly")
    out = tmp_path_factory.mktemp("isa")
    flags = _makefile_flags()
    srcs = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))

    def compile_one(src):
        dst = os.path.join(out, src + ".s")
        r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", src, "-o", dst], cwd=CSRC,
                           capture_output=True, text=True)
        assert r.returncode == 0, f"hipcc -S {src} failed:\n{r.stderr[-4000:]}"
        with open(dst) as f:
            return src, f.read()

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return dict(ex.map(compile_one, srcs))


def test_no_dpp_reads_a_fresh_packed_write(library_asm):
    bad, allowed, ndpp = [], [], 0
    for src, asm in library_asm.items():
        findings, n = check_asm(asm)
        ndpp += n
        for f in findings:
            (allowed if _allowed(f) else bad).append(f"{src}: {_fmt(f)}")
    # a parser that matches nothing must not pass: the library has thousands of DPP instructions
    assert ndpp >= 100, f"only {ndpp} DPP instructions found in {len(library_asm)} sources: the parser is broken"
    assert not bad, f"{len(bad)} DPP read(s) of a packed-FP32 write within {MIN_WAIT_STATES} wait states:\n" + "\n".join(bad)


def test_allowlist_entries_are_live(library_asm):
    # an allowlist entry that no longer matches anything is stale and must go
    for key in ALLOWLIST:
        hit = any(_allowed(f) and key[0] in f["function"] and key[1] in f["dpp"]
                  for asm in library_asm.values() for f in check_asm(asm)[0])
        assert hit, f"allowlist entry {key} matches no site"
