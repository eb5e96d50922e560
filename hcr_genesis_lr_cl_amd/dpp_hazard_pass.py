"""DPP read-after-write hazards of the kernels, settled on the compiler's assembly (hcr_genesis_lr_cl_amd/build.py runs this between
`hipcc -S` and the assembler for every kernel translation unit).

gfx9 does not interlock "VALU writes a VGPR -> a DPP instruction reads that VGPR as its DPP source": two wait states (issue slots of the
wave) have to lie between the two.  The compiler pads its own DPP instructions, but it does not look inside inline asm, and the
products of csrc/lg_quad.h (v_mul_f32_dpp / v_fmac_f32_dpp sequences) are inline asm: each block used to open with its own `s_nop 1`,
needed or not.  One wave per SIMD hides nothing: an `s_nop 1` is two issue slots, ~8.6 cycles (tools/ubench/pk_issue.hip), and the
physics loop had 50 of them per sub-step -- 1.0 us of the 25.6 us go2 step.

Only the DPP-routed operand (src0) is subject to the rule: a src1, the accumulator of v_fmac_f32_dpp (written and re-read in consecutive
slots throughout lg_quad.h's blocks) and the old destination of a masked DPP move are forwarded.  Every such form the built kernels contain
(hazard_classes) is a case of the on-chip table csrc/lg_dpp_kat.h (tests/test_gpu_dpp_operands.py), and mode='strict' -- two wait states
behind a write of ANY operand, LLVM's rule -- builds the reference library tests/test_gpu_dpp_strict_ab.py compares the product with.  The compiler pads for every VGPR operand of a
DPP instruction; where that padding stands in front of a plain f32 / mov DPP instruction and nothing nearby has wait-state rules of its
own (_blocks_relaxing: SGPR / VCC / EXEC writers, transcendentals, partial-register writes, memory, ...), it is dropped too
(`_relax_compiler_nops`: 44 of the loop's remaining wait states, another 0.4 us).

This pass removes those marked nops (`s_nop 1 ; lg-dpp-hazard`) and then walks every function: for EVERY `*_dpp` instruction -- the
compiler's and the asm blocks' alike -- it measures the wait states since the last VALU write of the DPP source register over all
paths that reach the instruction (branch targets resolved; an unknown predecessor counts as a write), and inserts exactly the `s_nop`
that is missing.  It also covers what the compiler cannot see in the other direction: a compiler-emitted DPP read right behind an asm
block that wrote its source ("VALU writes EXEC -> DPP", five wait states, is checked the same way).  The result never has fewer wait
states in front of a DPP read than the hardware asks for; `check()` re-verifies the rewritten text and the build fails on a finding.
"""
import re
import sys

MARK = "lg-dpp-hazard"
VGPR_DPP_WAIT = 2       # VALU writes VGPR -> DPP reads it
EXEC_DPP_WAIT = 5       # VALU writes EXEC -> DPP op

_LABEL = re.compile(r"^([.\w$]+):")
_REG = re.compile(r"^v(\d+)$")
_RANGE = re.compile(r"^v\[(\d+):(\d+)\]$")
_SDST = re.compile(r"^(vcc(_lo|_hi)?|s\d+|s\[\d+:\d+\])$")
_CTRL = re.compile(r"(quad_perm|row_|wave_|row_mirror|row_half_mirror)\S*(\s+(row_mask|bank_mask|bound_ctrl|fi)\S*)*")
# the DPP instructions whose operand layout roles() knows (vdst [, sdst], src0 [, src1 [, src2]]); any other *_dpp fails the build
DPP_MNEMONICS = frozenset(m + "_dpp" for m in (
    "v_mov_b32", "v_add_f32", "v_sub_f32", "v_subrev_f32", "v_mul_f32", "v_fmac_f32", "v_max_f32", "v_min_f32", "v_sqrt_f32",
    "v_or_b32", "v_and_b32", "v_xor_b32", "v_add_u32", "v_sub_u32", "v_add_co_u32", "v_sub_co_u32", "v_cndmask_b32"))


def _reads_old(text):
    """A DPP instruction leaves lanes unwritten -- and so reads its destination -- under a partial row / bank mask, or when its control
    can name a lane outside the row and bound_ctrl does not substitute zero."""
    code = text.split(";")[0]
    m = re.search(r"row_mask:(0x[0-9a-fA-F]+|\d+)", code)
    b = re.search(r"bank_mask:(0x[0-9a-fA-F]+|\d+)", code)
    if (m and int(m.group(1), 0) != 0xF) or (b and int(b.group(1), 0) != 0xF):
        return True
    always_valid = ("quad_perm", "row_ror", "row_mirror", "row_half_mirror")
    return "bound_ctrl" not in code and not any(c in code for c in always_valid)


class PassError(ValueError):
    """The instruction stream holds something the hazard model does not cover: the build stops."""


def _operands(rest):
    """Split the operand text at top-level commas; drop trailing modifiers (quad_perm:[..] row_mask:.. etc. stay attached to the last)."""
    out, depth, cur = [], 0, ""
    for ch in rest:
        if ch == "[":
            depth += 1
        elif ch == "]":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def _vgprs(op):
    """VGPR numbers named by one operand (`v12`, `-v12`, `|v12|`, `v[2:3]`), else an empty set."""
    op = op.split()[0] if op else ""
    op = op.strip("-|")
    if op.startswith("abs(") or op.startswith("neg("):
        op = op[4:].rstrip(")")
    m = _REG.match(op)
    if m:
        return {int(m.group(1))}
    m = _RANGE.match(op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


class Inst:
    __slots__ = ("mn", "ops", "line", "marked", "text")

    def __init__(self, mn, ops, line, marked, text):
        self.mn, self.ops, self.line, self.marked, self.text = mn, ops, line, marked, text

    @property
    def is_dpp(self):
        return self.mn.endswith("_dpp")

    @property
    def wait_states(self):
        if self.mn == "s_nop":
            return int(self.ops[0], 0) + 1 if self.ops else 1
        return 1

    def vgpr_writes(self):
        mn = self.mn
        if not mn.startswith("v_") or mn.startswith(("v_cmp", "v_readlane", "v_readfirstlane")):
            return set()
        w = _vgprs(self.ops[0]) if self.ops else set()
        if (mn.startswith("v_swap") or (mn.startswith("v_permlane") and "_swap" in mn)) and len(self.ops) > 1:
            w |= _vgprs(self.ops[1])        # both operands are written
        return w

    def writes_exec(self):
        return self.mn.startswith("v_cmpx") or (self.mn.startswith("v_") and bool(self.ops) and self.ops[0].split()[0] in ("exec", "exec_lo", "exec_hi"))

    def roles(self):
        """{role: VGPRs} of what this DPP instruction reads: 'dpp_src' (src0, routed across lanes), 'src1' / 'src2' (plain sources),
        'acc' (the destination of v_fmac / v_mac, read as the addend), 'old' (the destination's previous content, kept in the lanes a
        partial row / bank mask or an out-of-row source without bound_ctrl leaves unwritten).  SGPR / VCC destinations (carry-out) are
        skipped when locating src0."""
        ops, r = self.ops, {}
        k = 1
        while k < len(ops) and not _vgprs(ops[k]) and _SDST.match(ops[k].split()[0]):
            k += 1
        for role, j in (("dpp_src", k), ("src1", k + 1), ("src2", k + 2)):
            if j < len(ops):
                v = _vgprs(ops[j])
                if v:
                    r[role] = v
        dst = _vgprs(ops[0]) if ops else set()
        if self.mn.startswith(("v_fmac", "v_mac")):
            r["acc"] = dst
        elif dst and _reads_old(self.text):
            r["old"] = dst
        return r

    def dpp_source(self):
        return self.roles().get("dpp_src", set())

    def dpp_control(self):
        """The DPP modifiers as written (control, row / bank mask, bound_ctrl)."""
        m = _CTRL.search(self.text.split(";")[0])
        return " ".join(m.group(0).split()) if m else ""

    def branch_target(self):
        if self.mn.startswith(("s_cbranch", "s_branch")) and self.ops:
            return self.ops[0]
        return None


def _parse(lines):
    """-> list of functions; a function is a list of items: ('label', name, line) | Inst.  Only text between a global symbol label and
    its .Lfunc_end is a function."""
    funcs, cur = [], None
    for i, raw in enumerate(lines):
        s = raw.strip()
        if not s or s.startswith((";", "//")):
            continue
        m = _LABEL.match(s)
        if m:
            name = m.group(1)
            if name.startswith(".Lfunc_end"):
                if cur is not None:
                    funcs.append(cur)
                cur = None
            elif not name.startswith("."):
                cur = [("label", name, i)]
            elif cur is not None:
                cur.append(("label", name, i))
            continue
        if s.startswith(".") or cur is None:
            continue
        code = s.split(";")[0].split("//")[0].strip()
        if not code:
            continue
        parts = code.split(None, 1)
        mn = parts[0]
        ops = _operands(parts[1]) if len(parts) > 1 else []
        cur.append(Inst(mn, ops, i, MARK in s and mn == "s_nop", s))
    if cur is not None:
        funcs.append(cur)
    return funcs


def _recent_writes(items, idx, branches):
    """Every write that lies fewer wait states in front of the DPP instruction items[idx] than the hardware could ask for, over all paths
    that reach it: a list of (role, writer, wait states between).  role is one of the instruction's roles() ('dpp_src', 'src1', 'src2',
    'acc', 'old'; window: two wait states), 'exec' (a VALU write of EXEC; five) or 'unknown' (a predecessor the walk cannot follow: a
    label that no branch names and nothing falls through to, or more than eight branches deep; writer None -- it counts as a write of
    every operand)."""
    roles = items[idx].roles()
    found = []

    def walk(j, ws, depth):
        # scan backwards from item j (exclusive) with `ws` wait states already between
        while j > 0:
            j -= 1
            it = items[j]
            if isinstance(it, tuple):          # a label: whoever branches here is a predecessor too
                preds = branches.get(it[1], ())
                for b in preds:                # the branch instruction itself is one wait state
                    if depth < 8:
                        walk(b + 1, ws, depth + 1)
                    else:
                        found.append(("unknown", None, ws))
                if not preds and not _falls_into(items, j):
                    found.append(("unknown", None, ws))
                    return
                continue                       # ... and so is the fall-through path above the label (if it falls through)
            if it.mn == "s_branch" or it.mn == "s_endpgm" or it.mn.startswith("s_setpc"):
                return                         # nothing falls through an unconditional branch
            if ws < VGPR_DPP_WAIT:
                w = it.vgpr_writes()
                if w:
                    for role, regs in roles.items():
                        if w & regs:
                            found.append((role, it, ws))
            if ws < EXEC_DPP_WAIT and it.writes_exec():
                found.append(("exec", it, ws))
            ws += it.wait_states
            if ws >= EXEC_DPP_WAIT:
                return
        # ran off the top of the function with the window still open: the kernel entry, no writer before it
    walk(idx, 0, 0)
    return found


def _falls_into(items, j):
    """True when execution can fall through into the label items[j] from the instruction above it (or j is the function's entry)."""
    k = j - 1
    while k >= 0 and isinstance(items[k], tuple):
        k -= 1
    if k < 0:
        return True
    it = items[k]
    return not (it.mn in ("s_branch", "s_endpgm") or it.mn.startswith("s_setpc"))


STRICT_ROLES = ("dpp_src", "src1", "src2", "acc", "old")


def _needed(items, idx, branches, mode="default"):
    """Wait states missing in front of the DPP instruction items[idx] (0 = none).  mode 'default': the hardware rule as this project
    has measured it -- only a write of the DPP-routed source (and of EXEC) needs wait states; 'strict': LLVM's rule, two wait states
    behind a write of ANY VGPR operand (tests/test_gpu_dpp_strict_ab.py compares the two builds)."""
    roles = ("dpp_src",) if mode == "default" else STRICT_ROLES
    if mode not in ("default", "strict"):
        raise ValueError(f"dpp_hazard_pass: unknown mode {mode!r}")
    worst = 0
    for role, _, ws in _recent_writes(items, idx, branches):
        if role == "exec":
            worst = max(worst, EXEC_DPP_WAIT - ws)
        elif role in roles or role == "unknown":
            worst = max(worst, VGPR_DPP_WAIT - ws)
    return worst


def _analyse(items):
    """-> {label: [indices of the branches to it]}; fails on what the model does not cover (unknown DPP forms, indirect jumps)."""
    branches = {}
    for k, it in enumerate(items):
        if isinstance(it, Inst):
            if it.is_dpp and it.mn not in DPP_MNEMONICS:
                raise PassError(f"dpp_hazard_pass: {items[0][1]}: {it.mn} is not a DPP form the hazard model knows: {it.text}")
            if it.mn.startswith(("s_setpc", "s_swappc")):
                raise PassError(f"dpp_hazard_pass: {items[0][1]}: indirect jump ({it.text}): its targets are not known to the walk")
            t = it.branch_target()
            if t is not None:
                branches.setdefault(t, []).append(k)
    return branches


_PLAIN_DPP = ("v_mov_b32_dpp", "v_add_f32_dpp", "v_sub_f32_dpp", "v_subrev_f32_dpp", "v_mul_f32_dpp", "v_fmac_f32_dpp", "v_max_f32_dpp", "v_min_f32_dpp")
_TRANS = ("v_rcp", "v_rsq", "v_sqrt", "v_sin", "v_cos", "v_exp", "v_log")
RELAX_WINDOW = 6


def _blocks_relaxing(it):
    """True for anything in front of a compiler nop that could be the reason for it other than the DPP rule, or whose own consumers count
    wait states across it: VALU writes of SGPR / VCC / EXEC (lane selects, v_div_fmas, VMEM / VALU reads of that SGPR: up to 5 wait states),
    transcendental and partial-register (op_sel, SDWA, packed) results (forwarding hazards, 1 wait state), stores (their data registers
    may not be overwritten in the next slot), hardware-register accesses, and any instruction this pass does not know."""
    mn = it.mn
    if mn.startswith("v_"):
        if mn.startswith(("v_cmp", "v_readlane", "v_readfirstlane", "v_writelane", "v_div_", "v_mad_u64", "v_mad_i64", "v_mfma", "v_accvgpr", "v_permlane") + _TRANS):
            return True
        if "_co_" in mn or "_pk_" in mn or "sdwa" in mn or "op_sel" in it.text or "16" in mn:
            return True
        if it.ops and it.ops[0].split()[0].startswith(("s", "vcc", "exec", "a", "m0")):
            return True
        return False
    if mn in ("s_nop", "s_mov_b32", "s_mov_b64", "s_and_b64", "s_or_b64", "s_andn2_b64", "s_xor_b64", "s_add_i32", "s_sub_i32", "s_cmp_eq_u32", "s_cmp_lg_u32",
              "s_cselect_b32", "s_cselect_b64", "s_lshl_b32", "s_and_b32", "s_or_b32", "s_cmp_lt_i32", "s_cmp_ge_u32", "s_cmp_lg_u64", "s_mul_i32"):
        return False
    return True            # memory, branches, waitcnt, setreg, message, ... : leave the nop alone


def _relax_compiler_nops(lines, stats):
    """The compiler pads a DPP instruction when ANY of its VGPR operands was written in the two slots before; the hardware rule concerns the
    DPP-routed source only (the accumulators of lg_quad.h's blocks are written and re-read back to back).  Drop a compiler s_nop that stands
    directly in front of a plain f32 / mov DPP instruction when nothing in the RELAX_WINDOW instructions before it is of a kind that could
    need wait states for another reason (_blocks_relaxing) and no label lies in between; the main loop of fix() then re-inserts whatever
    the DPP source itself needs."""
    drop = set()
    for items in _parse(lines):
        for k, it in enumerate(items):
            if not (isinstance(it, Inst) and it.mn == "s_nop" and not it.marked and MARK not in it.text):
                continue
            nxt = items[k + 1] if k + 1 < len(items) else None
            if not (isinstance(nxt, Inst) and nxt.mn in _PLAIN_DPP):
                continue
            ok, j, seen = True, k, 0
            while seen < RELAX_WINDOW:
                j -= 1
                if j < 0 or isinstance(items[j], tuple) or _blocks_relaxing(items[j]):
                    ok = False
                    break
                seen += 1
            if ok:
                drop.add(it.line)
                stats["compiler_nops_relaxed"] += 1
                stats["compiler_wait_states_relaxed"] += it.wait_states
    return [raw for i, raw in enumerate(lines) if i not in drop]


def fix(text, relax=True, mode="default"):
    """-> (new text, stats).  mode 'default': removes the marked nops (and, `relax`, the compiler's over-wide padding in front of plain DPP
    instructions), then inserts the minimal s_nop in front of every DPP read whose DPP source needs one.  mode 'strict': removes and relaxes
    nothing and pads every DPP read to two wait states behind a write of any of its VGPR operands, inside asm blocks too."""
    if mode == "strict":
        relax = False
    lines = text.split("\n")
    stats = {"marked": 0, "kept_or_inserted": 0, "wait_states_inserted": 0, "dpp": 0, "functions": 0, "compiler_nops_relaxed": 0, "compiler_wait_states_relaxed": 0}
    # 1. drop the marked nops
    keep = []
    for raw in lines:
        s = raw.strip()
        if mode == "default" and MARK in s and s.startswith("s_nop"):
            stats["marked"] += 1
            continue
        keep.append(raw)
    lines = keep
    if relax:
        lines = _relax_compiler_nops(lines, stats)
    # 2. insert what is missing, function by function, top to bottom (an insertion only lengthens later distances)
    funcs = _parse(lines)
    stats["functions"] = len(funcs)
    inserts = {}                                # line index -> s_nop operand
    for items in funcs:
        branches = _analyse(items)
        k = 0
        while k < len(items):
            it = items[k]
            if isinstance(it, Inst) and it.is_dpp:
                stats["dpp"] += 1
                need = _needed(items, k, branches, mode)
                if need > 0:
                    nop = Inst("s_nop", [str(need - 1)], it.line, False, "")
                    items.insert(k, nop)
                    # branch indices behind k shift by one
                    for t in branches:
                        branches[t] = [b + 1 if b >= k else b for b in branches[t]]
                    inserts[it.line] = max(inserts.get(it.line, 0), need)
                    stats["kept_or_inserted"] += 1
                    stats["wait_states_inserted"] += need
                    k += 1
            k += 1
    out = []
    for i, raw in enumerate(lines):
        if i in inserts:
            out.append(f"\ts_nop {inserts[i] - 1} ; {MARK} (pass)")
        out.append(raw)
    return "\n".join(out), stats


def check(text, mode="default"):
    """Findings (function, line number, instruction, missing wait states) of a text as it stands under `mode`'s rule; [] = clean."""
    lines = text.split("\n")
    bad = []
    for items in _parse(lines):
        branches = _analyse(items)
        for k, it in enumerate(items):
            if isinstance(it, Inst) and it.is_dpp:
                need = _needed(items, k, branches, mode)
                if need > 0:
                    bad.append((items[0][1], it.line + 1, it.text, need))
    return bad


def check_strict(text):
    return check(text, mode="strict")


def writer_kind(it):
    """'dpp' (a DPP VALU), 'trans' (a transcendental), 'valu' (any other VALU); 'unknown' for an unresolved predecessor."""
    if it is None:
        return "unknown"
    if it.is_dpp:
        return "dpp"
    if it.mn.startswith(_TRANS):
        return "trans"
    return "valu"


def hazard_classes(text):
    """{(mnemonic, role, writer kind, wait states, control): count} of the DPP reads in `text` that have an operand written fewer than two
    wait states before (over all paths, as fix() walks them) -- the forms the chip has to forward for the default rule to hold."""
    out = {}
    for items in _parse(text.split("\n")):
        branches = _analyse(items)
        for k, it in enumerate(items):
            if isinstance(it, Inst) and it.is_dpp:
                seen = set()
                for role, w, ws in _recent_writes(items, k, branches):
                    if role == "exec" or ws >= VGPR_DPP_WAIT:
                        continue
                    key = (it.mn, role, writer_kind(w), ws, it.dpp_control())
                    if key not in seen:
                        seen.add(key)
                        out[key] = out.get(key, 0) + 1
    return out


if __name__ == "__main__":
    src = open(sys.argv[1]).read()
    if len(sys.argv) > 2 and sys.argv[2] == "--check":
        f = check(src)
        for x in f[:50]:
            print(x)
        print(len(f), "finding(s)")
        sys.exit(1 if f else 0)
    new, st = fix(src)
    print(st, "findings after:", len(check(new)))
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(new)
