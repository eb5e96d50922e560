"""The build's DPP hazard pass (hcr_genesis_lr_cl_amd/dpp_hazard_pass.py) on hand-written instruction streams: it may only ever remove a
wait state that the hardware rule "VALU writes VGPR -> DPP source read: 2 wait states" does not ask for."""
import glob
import json
import os
import re
import subprocess

import numpy as np
import pytest

from hcr_genesis_lr_cl_amd import dpp_hazard_pass as P
from hcr_genesis_lr_cl_amd import dpp_kat as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QP = "quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf"


def kernel(body):
    return "\t.text\nk:\n" + "\n".join("\t" + l if not l.endswith(":") else l for l in body) + "\n.Lfunc_end0:\n"


def nops(text):
    return [l.strip().split(";")[0].strip() for l in text.split("\n") if l.strip().startswith("s_nop")]


def test_marked_nop_goes_when_the_source_is_old():
    src = kernel(["v_mul_f32_e32 v5, v1, v2", "v_add_f32_e32 v6, v1, v2", "v_add_f32_e32 v7, v1, v2",
                  "s_nop 1 ; lg-dpp-hazard", f"v_mul_f32_dpp v9, v5, v3 {QP}", "s_endpgm"])
    out, st = P.fix(src)
    assert nops(out) == [] and st["marked"] == 1 and st["kept_or_inserted"] == 0
    assert P.check(out) == []


def test_marked_nop_stays_when_the_source_was_just_written():
    src = kernel(["v_mul_f32_e32 v5, v1, v2", "s_nop 1 ; lg-dpp-hazard", f"v_mul_f32_dpp v9, v5, v3 {QP}", "s_endpgm"])
    out, st = P.fix(src)
    assert nops(out) == ["s_nop 1"] and P.check(out) == []


def test_one_instruction_in_between_leaves_one_wait_state_to_pad():
    src = kernel(["v_mul_f32_e32 v5, v1, v2", "v_add_f32_e32 v6, v1, v2", "s_nop 1 ; lg-dpp-hazard", f"v_fmac_f32_dpp v9, v5, v3 {QP}", "s_endpgm"])
    out, _ = P.fix(src)
    assert nops(out) == ["s_nop 0"] and P.check(out) == []


def test_only_the_dpp_routed_operand_counts():
    # v3 (plain operand) and v9 (accumulator) are fresh, the DPP source v5 is old: nothing to pad
    src = kernel(["v_mul_f32_e32 v5, v1, v2", "v_add_f32_e32 v6, v1, v2", "v_mul_f32_e32 v3, v1, v2", "v_mul_f32_e32 v9, v1, v2",
                  "s_nop 1 ; lg-dpp-hazard", f"v_fmac_f32_dpp v9, v5, v3 {QP}", "s_endpgm"])
    out, _ = P.fix(src)
    assert nops(out) == []


def test_a_write_inside_a_register_pair_is_seen():
    src = kernel(["v_pk_fma_f32 v[4:5], v[0:1], v[2:3], v[6:7]", "s_nop 1 ; lg-dpp-hazard", f"v_mov_b32_dpp v9, v5 {QP}", "s_endpgm"])
    out, _ = P.fix(src)
    assert nops(out) == ["s_nop 1"]


def test_a_branch_into_the_block_is_a_predecessor():
    # fall-through path: v5 written three instructions before; the branch path writes it right before jumping
    src = kernel(["v_mul_f32_e32 v5, v1, v2", "s_cbranch_scc1 .LBB0_2", "v_add_f32_e32 v6, v1, v2", "v_add_f32_e32 v7, v1, v2", "v_add_f32_e32 v8, v1, v2",
                  ".LBB0_2:", "s_nop 1 ; lg-dpp-hazard", f"v_mul_f32_dpp v9, v5, v3 {QP}", "s_endpgm"])
    out, _ = P.fix(src)
    assert nops(out) == ["s_nop 0"]          # write, branch (one wait state), DPP read: one more is missing on that path
    assert P.check(out) == []


def test_compiler_visible_dpp_behind_an_asm_write_is_padded():
    src = kernel([f"v_fmac_f32_dpp v9, v5, v3 {QP}", f"v_mov_b32_dpp v10, v9 {QP}", "s_endpgm"])
    assert len(P.check(src)) == 1
    out, st = P.fix(src)
    assert nops(out) == ["s_nop 1"] and st["kept_or_inserted"] == 1 and P.check(out) == []


def test_exec_written_by_a_valu_compare_needs_five():
    src = kernel(["v_cmpx_lt_f32_e32 v1, v2", "v_add_f32_e32 v6, v1, v2", f"v_mov_b32_dpp v10, v9 {QP}", "s_endpgm"])
    out, _ = P.fix(src)
    assert nops(out) == ["s_nop 3"] and P.check(out) == []    # five wait states, one instruction already in between


def test_unmarked_nops_are_left_alone_and_counted():
    src = kernel(["v_mul_f32_e32 v5, v1, v2", "s_nop 0", f"v_mul_f32_dpp v9, v5, v3 {QP}", "s_endpgm"])
    out, _ = P.fix(src)
    assert nops(out) == ["s_nop 0", "s_nop 0"]   # the compiler's one wait state stays, the missing one is added


FILL = ["v_add_f32_e32 v20, v1, v2", "v_add_f32_e32 v21, v1, v2", "v_add_f32_e32 v22, v1, v2", "v_add_f32_e32 v23, v1, v2", "v_add_f32_e32 v24, v1, v2",
        "v_add_f32_e32 v25, v1, v2"]


def test_compiler_padding_for_a_plain_operand_is_dropped():
    # the compiler's s_nop 1 is there because v60 (PLAIN operand of the DPP add) was just written; the DPP source v59 is old
    src = kernel(FILL + ["v_mul_f32_e32 v59, v1, v2", "v_add_f32_e32 v30, v1, v2", "v_add_f32_e32 v60, v1, v2", "s_nop 1",
                         "v_add_f32_dpp v61, v59, v60 quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1", "s_endpgm"])
    out, st = P.fix(src)
    assert nops(out) == [] and st["compiler_nops_relaxed"] == 1 and st["compiler_wait_states_relaxed"] == 2
    assert nops(P.fix(src, relax=False)[0]) == ["s_nop 1"]


def test_compiler_padding_comes_back_when_the_dpp_source_needs_it():
    src = kernel(FILL + ["v_mul_f32_e32 v59, v1, v2", "s_nop 1", "v_add_f32_dpp v61, v59, v60 quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1", "s_endpgm"])
    out, st = P.fix(src)
    assert nops(out) == ["s_nop 1"] and st["compiler_nops_relaxed"] == 1 and st["kept_or_inserted"] == 1


@pytest.mark.parametrize("blocker", ["v_cmp_lt_f32_e32 vcc, v1, v2", "v_rcp_f32_e32 v40, v1", "v_readlane_b32 s6, v18, 0", "global_store_dword v1, v2, s[0:1]",
                                     "v_pk_fma_f32 v[40:41], v[0:1], v[2:3], v[6:7]", "s_waitcnt vmcnt(0)", "v_add_co_u32_e32 v40, vcc, v1, v2"])
def test_compiler_padding_is_left_alone_next_to_anything_with_rules_of_its_own(blocker):
    src = kernel(FILL + [blocker, "v_add_f32_e32 v30, v1, v2", "v_add_f32_e32 v60, v1, v2", "s_nop 1",
                         "v_add_f32_dpp v61, v59, v60 quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1", "s_endpgm"])
    out, st = P.fix(src)
    assert nops(out) == ["s_nop 1"] and st["compiler_nops_relaxed"] == 0


def test_compiler_padding_is_left_alone_behind_a_label_and_in_front_of_other_instructions():
    src = kernel(FILL[:3] + [".LBB0_4:"] + FILL[:3] + ["s_nop 1", "v_add_f32_dpp v61, v59, v60 quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf bound_ctrl:1", "s_endpgm"])
    assert nops(P.fix(src)[0]) == ["s_nop 1"]
    src = kernel(FILL + ["s_nop 0", "v_cndmask_b32_dpp v61, v59, v60, vcc quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf", "s_endpgm"])
    assert nops(P.fix(src)[0]) == ["s_nop 0"]
    src = kernel(FILL + ["s_nop 0", "v_mul_f32_e32 v61, v59, v60", "s_endpgm"])
    assert nops(P.fix(src)[0]) == ["s_nop 0"]


def test_the_built_library_went_through_the_pass():
    side = os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc", "liblgsim.build.json")
    if not os.path.exists(side):
        pytest.skip("library not built")
    with open(side) as f:
        meta = json.load(f)
    st = meta.get("dpp_hazard_pass")
    assert st and st["marked"] > 0 and st["dpp"] > 10000, st
    # whatever the pass wrote next to the objects is clean under its own check (these files stay in the build tree)
    for path in glob.glob(os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc", "obj", "lg_inst_*.fix.s"))[:3]:
        with open(path) as f:
            assert P.check(f.read()) == [], path


# ---- the operand-role model, the model's limits, and the strict mode ----

def test_operand_roles():
    roles = lambda t: P._parse(kernel([t]).split("\n"))[0][1].roles()
    assert roles(f"v_fmac_f32_dpp v9, v5, v3 {QP}") == {"dpp_src": {5}, "src1": {3}, "acc": {9}}
    assert roles(f"v_add_f32_dpp v9, -v5, |v3| {QP}") == {"dpp_src": {5}, "src1": {3}}
    assert roles("v_mov_b32_dpp v9, v5 row_shr:4 row_mask:0xf bank_mask:0xa") == {"dpp_src": {5}, "old": {9}}     # masked banks keep v9
    assert roles("v_mov_b32_dpp v9, v5 row_shl:1 row_mask:0xf bank_mask:0xf") == {"dpp_src": {5}, "old": {9}}     # lane 15 of a row keeps v9
    assert roles("v_mov_b32_dpp v9, v5 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1") == {"dpp_src": {5}}
    assert roles("v_cndmask_b32_dpp v9, v5, v3, vcc quad_perm:[2,0,1,3] row_mask:0xf bank_mask:0xf") == {"dpp_src": {5}, "src1": {3}}


def test_src0_is_found_behind_a_carry_out():
    # v_add_co_u32_dpp v9, vcc, v5, v3: ops[1] is the carry-out, the DPP source is v5
    src = kernel(["v_mul_f32_e32 v5, v1, v2", "v_add_co_u32_dpp v9, vcc, v5, v3 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf", "s_endpgm"])
    assert P._parse(src.split("\n"))[0][2].dpp_source() == {5}
    out, _ = P.fix(src)
    assert nops(out) == ["s_nop 1"] and P.check(out) == []
    src = kernel(["v_mul_f32_e32 v3, v1, v2", "v_add_co_u32_dpp v9, vcc, v5, v3 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf", "s_endpgm"])
    assert nops(P.fix(src)[0]) == []              # vcc is not mistaken for the source, v3 is src1


def test_a_dpp_form_the_model_does_not_know_fails_the_build():
    src = kernel([f"v_max_i32_dpp v9, v5, v3 {QP}", "s_endpgm"])
    with pytest.raises(P.PassError, match="v_max_i32_dpp"):
        P.fix(src)
    with pytest.raises(P.PassError):
        P.check(src)


@pytest.mark.parametrize("jump", ["s_setpc_b64 s[4:5]", "s_swappc_b64 s[30:31], s[4:5]"])
def test_an_indirect_jump_fails_the_build(jump):
    src = kernel(["v_mul_f32_e32 v5, v1, v2", jump, f"v_mov_b32_dpp v9, v5 {QP}", "s_endpgm"])
    with pytest.raises(P.PassError, match="indirect"):
        P.fix(src)


def test_a_label_nothing_is_known_to_reach_counts_as_an_immediate_writer():
    # .LBB0_2 follows an unconditional branch and no branch names it: whoever gets there (a jump table, say) may just have written v5
    src = kernel(["v_mul_f32_e32 v5, v1, v2", "v_add_f32_e32 v6, v1, v2", "v_add_f32_e32 v7, v1, v2", "s_branch .LBB0_3", ".LBB0_2:",
                  f"v_mov_b32_dpp v9, v5 {QP}", ".LBB0_3:", "s_endpgm"])
    out, _ = P.fix(src)
    assert nops(out) == ["s_nop 1"] and P.check(out) == []
    # the same label reached by a branch from far enough away is fine
    src = kernel(["s_cbranch_scc1 .LBB0_2", "v_mul_f32_e32 v5, v1, v2", "v_add_f32_e32 v6, v1, v2", "s_branch .LBB0_3", ".LBB0_2:",
                  f"v_mov_b32_dpp v9, v5 {QP}", ".LBB0_3:", "s_endpgm"])
    assert nops(P.fix(src)[0]) == []


def test_a_permlane_swap_writes_both_operands():
    src = kernel(["v_permlane32_swap_b32_e32 v4, v5", f"v_mov_b32_dpp v9, v5 {QP}", "s_endpgm"])
    out, _ = P.fix(src)
    assert nops(out) == ["s_nop 1"] and P.check(out) == []


def test_strict_mode_pads_a_fresh_accumulator_and_a_fresh_plain_operand():
    src = kernel(["v_mul_f32_e32 v9, v1, v2", f"v_fmac_f32_dpp v9, v5, v3 {QP}",        # fresh accumulator
                  "v_mul_f32_e32 v3, v1, v2", f"v_add_f32_dpp v10, v6, v3 {QP}",         # fresh src1
                  "v_mov_b32_e32 v11, v1", "s_nop 1 ; lg-dpp-hazard", f"v_mov_b32_dpp v12, v7 {QP}", "s_endpgm"])
    assert nops(P.fix(src)[0]) == []                                       # the default rule: src0 is old everywhere, the marked nop goes
    out, st = P.fix(src, mode="strict")
    assert nops(out) == ["s_nop 1", "s_nop 1", "s_nop 1"]                   # two inserted, the marked one kept: strict removes nothing
    assert st["kept_or_inserted"] == 2 and st["compiler_nops_relaxed"] == 0
    assert P.check_strict(out) == []


def test_check_strict_reports_the_forwarded_reads_of_the_default_output():
    src = kernel(["v_mul_f32_e32 v9, v1, v2", f"v_fmac_f32_dpp v9, v5, v3 {QP}", "v_mul_f32_e32 v3, v1, v2", f"v_add_f32_dpp v10, v6, v3 {QP}",
                  "s_endpgm"])
    out, _ = P.fix(src)
    assert P.check(out) == []
    bad = P.check_strict(out)
    assert [b[2].split()[0] for b in bad] == ["v_fmac_f32_dpp", "v_add_f32_dpp"] and all(b[3] == 2 for b in bad)
    assert set(P.hazard_classes(out)) == {("v_fmac_f32_dpp", "acc", "valu", 0, QP), ("v_add_f32_dpp", "src1", "valu", 0, QP)}


# ---- the on-chip known-answer table (csrc/lg_dpp_kat.h) ----

def _kat_kernel_text(case):
    regs = {"%[x]": "v1", "%[y]": "v2", "%[z]": "v3", "%[s]": "v4", "%[o]": "v5", "%[d]": "v6", "%[r]": "v7", "%[t]": "v8"}
    body = []
    for line in K.PROLOGUE + case.lines + K.EPILOGUE:
        for k, v in regs.items():
            line = line.replace(k, v)
        body.append(line)
    return kernel(body + ["s_endpgm"])


def test_every_kat_case_is_the_form_its_table_entry_names():
    table = K.cases()
    assert len(table) > 200
    for c in table:
        want = {c.key()} if c.dist < K.WAITED else set()
        assert set(P.hazard_classes(_kat_kernel_text(c))) == want, c


def test_every_kat_case_would_notice_a_stale_read_and_no_correct_result_equals_a_sentinel():
    inp = K.inputs()
    ref = K.reference(K.cases(), inp)
    assert not np.isin(ref, inp[3]).any()
    assert np.all(ref == np.round(ref * 2) / 2) and np.abs(ref).max() < 2 ** 20        # exact in f32
    for c in K.cases():
        fresh, stale = K.run_case(c, inp), K.run_case(c, inp, stale=True)
        assert np.any((fresh["d"] != stale["d"]) | (fresh["r"] != stale["r"])), c


def test_the_kat_keeps_the_three_original_positive_checks():
    keys = {c.key() for c in K.cases()}
    c1 = "quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf"
    assert ("v_add_f32_dpp", "src1", "valu", 0, c1) in keys            # a plain operand written in the slot before
    assert ("v_fmac_f32_dpp", "acc", "valu", 0, c1) in keys            # the accumulator likewise
    assert ("v_add_f32_dpp", "dpp_src", "valu", K.WAITED, c1) in keys  # a fresh DPP source behind `s_nop 1`


LLVM_BIN = os.environ.get("LG_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
CSRC = os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc")


def _disassemble(obj, tmp_path):
    """[(function, [(address, instruction text, branch target address or None)])] of the gfx950 code object embedded in a host object."""
    tag = os.path.basename(os.path.dirname(obj)) + "_" + os.path.basename(obj)
    fb, co = str(tmp_path / (tag + ".fatbin")), str(tmp_path / (tag + ".co"))
    subprocess.run([os.path.join(LLVM_BIN, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + fb, obj, str(tmp_path / (tag + ".host"))], check=True)
    subprocess.run([os.path.join(LLVM_BIN, "clang-offload-bundler"), "-type=o", "-targets=hipv4-amdgcn-amd-amdhsa--gfx950", "-input=" + fb,
                    "-output=" + co, "-unbundle"], check=True)
    text = subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", "--mcpu=gfx950", co], check=True, capture_output=True, text=True).stdout
    funcs, cur, start = [], None, 0
    for line in text.split("\n"):
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            cur = (m.group(2), [])
            start = int(m.group(1), 16)
            funcs.append(cur)
            continue
        m = re.match(r"^\s+(\S.*?)\s*// ([0-9A-F]+): ([0-9A-F ]+?)\s*(<(.+)\+0x([0-9a-f]+)>)?$", line)
        if m and cur is not None:
            target = start + int(m.group(6), 16) if m.group(6) and m.group(5) == cur[0] else None
            cur[1].append((int(m.group(2), 16), m.group(1), target, m.group(3)))
    for _, insts in funcs:       # alignment padding behind the last instruction (zero words; objdump prints a lone one as an instruction)
        while insts and insts[-1][3] == "00000000":
            insts.pop()
    return [(n, [i[:3] for i in insts]) for n, insts in funcs]


def _without_nops(insts):
    """The instruction texts with every s_nop removed and branch offsets replaced by the index of the (non-nop) instruction they reach."""
    kept = [(a, t, tg) for a, t, tg in insts if not t.startswith("s_nop")]
    index = {a: k for k, (a, _, _) in enumerate(kept)}
    addrs = sorted(index)
    out = []
    for a, t, tg in kept:
        if tg is not None:
            nxt = next((x for x in addrs if x >= tg), None)
            t = t.split()[0] + f" -> {index.get(nxt)}"
        out.append(t)
    return out


def _kat_asm_lines(case):
    return K.PROLOGUE + case.lines + K.EPILOGUE


def test_the_built_kat_kernel_runs_every_case_exactly_as_written(tmp_path):
    obj = os.path.join(CSRC, "obj", "lg_host.o")
    if not os.path.exists(obj):
        pytest.skip("library not built")
    funcs = {name: insts for name, insts in _disassemble(obj, tmp_path)}
    name = next(n for n in funcs if "dpp_kat_table_kernel" in n)
    insts = [" ".join(t.replace(",", " ").split()) for _, t, _ in funcs[name]]
    pos = 0
    for c in K.cases():
        want = [" ".join(l.replace(",", " ").split()) for l in _kat_asm_lines(c)]
        found = None
        for k in range(pos, len(insts) - len(want) + 1):
            if insts[k] != "s_nop 4":
                continue
            binding, ok = {}, True
            for w, got in zip(want, insts[k:k + len(want)]):
                wre = "^" + re.sub(r"%\\\[(\w)\\\]", r"(?P<\1>v\\d+)", re.escape(w)) + "$"
                m = re.match(wre, got)
                if not m or any(binding.setdefault(n, v) != v for n, v in m.groupdict().items()):
                    ok = False
                    break
            if ok:
                found = k
                break
        assert found is not None, f"{c}: not found in the disassembly exactly as written: {want}"
        pos = found + len(want)


def test_the_strict_library_differs_from_the_product_only_in_s_nops(tmp_path):
    prod, strict = os.path.join(CSRC, "liblgsim.build.json"), os.path.join(CSRC, "liblgsim_strict.build.json")
    if not (os.path.exists(prod) and os.path.exists(strict)):
        pytest.skip("libraries not built")
    with open(prod) as f:
        mp = json.load(f)
    with open(strict) as f:
        ms = json.load(f)
    assert mp["source_hash"] == ms["source_hash"] and mp["flags"] == ms["flags"]
    assert mp["dpp_pass_mode"] == "default" and ms["dpp_pass_mode"] == "strict"
    n_prod = n_strict = 0
    for g in range(22):
        sp = os.path.join(CSRC, "obj", f"lg_inst_{g}.fix.s")
        ss = os.path.join(CSRC, "obj_liblgsim_strict", f"lg_inst_{g}.fix.s")
        with open(ss) as f:
            assert P.check_strict(f.read()) == [], ss
        with open(sp) as f:
            n_prod += len(P.check_strict(f.read()))
        a = _disassemble(os.path.join(CSRC, "obj", f"lg_inst_{g}.o"), tmp_path)
        b = _disassemble(os.path.join(CSRC, "obj_liblgsim_strict", f"lg_inst_{g}.o"), tmp_path)
        assert [n for n, _ in a] == [n for n, _ in b], g
        for (name, ia), (_, ib) in zip(a, b):
            assert _without_nops(ia) == _without_nops(ib), (g, name)
            n_strict += sum(t.startswith("s_nop") for _, t, _ in ib) - sum(t.startswith("s_nop") for _, t, _ in ia)
    assert n_prod > 1000          # the product forwards thousands of operands the strict build waits for
    assert n_strict > 0


def test_every_forwarded_form_of_the_kernels_is_a_kat_case():
    side = os.path.join(CSRC, "liblgsim.build.json")
    if not os.path.exists(side):
        pytest.skip("library not built")
    covered = {c.key() for c in K.cases()}
    seen = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "obj", "lg_inst_*.fix.s"))):
        with open(path) as f:
            for k, v in P.hazard_classes(f.read()).items():
                seen[k] = seen.get(k, 0) + v
    assert seen, "no forwarded DPP operand at all: the classification found nothing to check"
    missing = sorted(k for k in seen if k not in covered)
    assert missing == [], "forwarded DPP forms with no case in csrc/lg_dpp_kat.h:\n" + "\n".join(f"{seen[k]:6d} {k}" for k in missing)
