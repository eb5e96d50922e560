"""Builds csrc/liblgsim.so with hipcc for gfx950 (in-tree, so it travels to the GPU box).

The library is 36 translation units: lg_host.hip (C ABI), lg_rollout.hip, lg_sensor.hip, lg_policy.hip, lg_ppo.hip, lg_optim.hip, lg_train.hip, lg_train_ee.hip, lg_train_ts.hip, lg_train_dwaq.hip, lg_train_cts.hip, lg_train_rnn.hip, lg_train_tcn.hip, lg_runner.hip and lg_inst.hip compiled once per
kernel-instantiation group (-DLG_GROUP=0..21).  They are compiled in parallel into csrc/obj/ and linked; an object is reused while the sources it depends on and
the flags are unchanged (content hash), so an edit of lg_quad.h rebuilds the twelve component-per-lane groups only.

The kernel groups go through the compiler's ASSEMBLY: hipcc -S (device) -> dpp_hazard_pass.fix (the s_nop each DPP read needs, no
more: the inline-asm products of lg_quad.h otherwise pay a two-slot nop per block) -> assembler -> lld -> offload bundle -> host
compile with that bundle.  These are the steps `hipcc -c` runs itself (hipcc -###), with the pass in the middle; the rewritten text is
re-checked and a finding fails the build.  LG_NO_DPP_PASS=1 compiles the groups with plain `hipcc -c` (every marked nop stays).
LG_DPP_PASS_MODE=strict runs the pass in its strict mode (LLVM's rule: two wait states behind a write of ANY VGPR operand of a DPP
instruction, asm blocks included, nothing removed); __graft_entry__.build() builds csrc/liblgsim_strict.so that way next to the product
library, and tests/test_gpu_dpp_strict_ab.py compares the two."""
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INC = os.path.join(HERE, "..", "include")
# LG_BUILD_OUT: a developer variant (other flags, e.g. -DLG_DBG_STAMPS) next to the product library; load it with LG_LIB=<path>
OUT = os.environ.get("LG_BUILD_OUT") or os.path.join(CSRC, "liblgsim.so")
OBJ = os.path.join(CSRC, "obj" if "LG_BUILD_OUT" not in os.environ else "obj_" + os.path.splitext(os.path.basename(OUT))[0])
LLVM_BIN = os.environ.get("LG_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
DPP_PASS = os.environ.get("LG_NO_DPP_PASS", "0") != "1"
PASS_MODE = os.environ.get("LG_DPP_PASS_MODE", "default")
if PASS_MODE not in ("default", "strict"):
    raise ValueError(f"LG_DPP_PASS_MODE={PASS_MODE!r}: expected 'default' or 'strict'")
N_GROUPS = 22
QUAD_GROUPS = list(range(0, 9)) + list(range(17, 22))   # lg_inst.hip: groups that include lg_quad.h
COMMON = ["lg_shared.h", "lg_math.h", "lg_lane_ints.h", os.path.join(INC, "lgsim.h")]
# -fno-slp-vectorize: packing scalars into v_pk_* costs more v_mov / AGPR shuffles than it saves here.
# iterative-ilp scheduling: the kernels run one wave per SIMD, so occupancy is irrelevant and the scheduler should fill DPP /
# VALU->SGPR hazard slots with independent work (measured -3 % on the physics launch, neutral elsewhere).
EXTRA_FLAGS = os.environ.get("LG_HIPCC_FLAGS", "-fno-slp-vectorize -mllvm -amdgpu-sched-strategy=iterative-ilp").split()
SIDECAR = os.path.splitext(OUT)[0] + ".build.json"
FALLBACK_FLAGS = [["-fno-slp-vectorize", "-mllvm", "-amdgpu-sched-strategy=max-ilp"], ["-fno-slp-vectorize"]]


def units():
    """(object name, source, extra defines, dependencies) of every translation unit."""
    u = [("lg_host", "lg_host.hip", [], COMMON + ["lg_dpp_kat.h"]), ("lg_rollout", "lg_rollout.hip", [], [os.path.join(INC, "lgrollout.h")]),
         ("lg_sensor", "lg_sensor.hip", [], [os.path.join(INC, "lgsensor.h")]),
         ("lg_policy", "lg_policy.hip", [], ["lg_math.h", os.path.join(INC, "lgpolicy.h")]),
         ("lg_ppo", "lg_ppo.hip", [], [os.path.join(INC, "lgppo.h")]),
         ("lg_optim", "lg_optim.hip", [], [os.path.join(INC, "lgoptim.h")]),
         ("lg_train", "lg_train.hip", [], [os.path.join(INC, "lgtrain.h"), os.path.join(INC, "lgpolicy.h"), "lg_train_tiles.h", "lg_train_pass.h"]),
         ("lg_train_ee", "lg_train_ee.hip", [], [os.path.join(INC, "lgtrainee.h"), os.path.join(INC, "lgtrain.h"), os.path.join(INC, "lgpolicy.h"),
                                                 "lg_train_tiles.h", "lg_train_pass.h"]),
         ("lg_train_ts", "lg_train_ts.hip", [], [os.path.join(INC, "lgtraints.h"), os.path.join(INC, "lgtrain.h"), os.path.join(INC, "lgpolicy.h"),
                                                 "lg_train_tiles.h", "lg_train_pass.h"]),
         ("lg_train_dwaq", "lg_train_dwaq.hip", [], [os.path.join(INC, "lgtraindwaq.h"), os.path.join(INC, "lgtrain.h"), os.path.join(INC, "lgpolicy.h"),
                                                     "lg_train_tiles.h", "lg_train_pass.h"]),
         ("lg_train_cts", "lg_train_cts.hip", [], [os.path.join(INC, "lgtraincts.h"), os.path.join(INC, "lgtraints.h"), os.path.join(INC, "lgtrain.h"),
                                                   os.path.join(INC, "lgpolicy.h"), "lg_train_tiles.h", "lg_train_pass.h"]),
         ("lg_train_rnn", "lg_train_rnn.hip", [], [os.path.join(INC, "lgtrainrnn.h"), os.path.join(INC, "lgtrain.h"), os.path.join(INC, "lgpolicy.h"),
                                                   "lg_train_tiles.h", "lg_train_pass.h"]),
         ("lg_train_tcn", "lg_train_tcn.hip", [], [os.path.join(INC, "lgtraintcn.h"), os.path.join(INC, "lgtrain.h"), os.path.join(INC, "lgpolicy.h"),
                                                   "lg_train_tiles.h", "lg_train_pass.h"]),
         ("lg_runner", "lg_runner.hip", [], [os.path.join(INC, "lgrunner.h")])]
    for g in range(N_GROUPS):
        deps = COMMON + ["lg_kernel.h"] + (["lg_quad.h"] if g in QUAD_GROUPS else []) + ([os.path.join(HERE, "dpp_hazard_pass.py")] if DPP_PASS else [])
        u.append((f"lg_inst_{g}", "lg_inst.hip", [f"-DLG_GROUP={g}"], deps))
    return u


def _path(f):
    return f if os.path.isabs(f) else os.path.join(CSRC, f)


def source_hash():
    """Hash of every source the library is built from (csrc/*.hip, csrc/*.h, include/*.h): stamps profiles and the build sidecar."""
    h = hashlib.sha256()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    files += sorted(os.path.join(INC, f) for f in os.listdir(INC) if f.endswith(".h"))
    if DPP_PASS:
        files.append(os.path.join(HERE, "dpp_hazard_pass.py"))     # it rewrites the kernels' instruction stream
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _unit_key(src, defs, deps, flags):
    h = hashlib.sha256(" ".join(flags + defs + (["dpp-pass", PASS_MODE] if DPP_PASS else [])).encode())
    for f in [src] + list(deps):
        with open(_path(f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def needs_build():
    if not os.path.exists(OUT):
        return True
    try:
        with open(SIDECAR) as f:
            return json.load(f).get("source_hash") != source_hash()
    except (OSError, ValueError):
        return True


def _compile_all(hipcc, flags, force, jobs, verbose):
    """Compile every stale unit (in parallel); returns (object paths, first error text or '')."""
    os.makedirs(OBJ, exist_ok=True)
    todo, objs = [], []
    for name, src, defs, deps in units():
        obj, keyf = os.path.join(OBJ, name + ".o"), os.path.join(OBJ, name + ".key")
        key = _unit_key(src, defs, deps, flags)
        objs.append(obj)
        old = open(keyf).read() if os.path.exists(keyf) and os.path.exists(obj) else ""
        if force or old != key:
            base = [hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", *flags, *defs]
            cmd = [*base, "-c", _path(src), "-o", obj]
            todo.append((name, ("pass", base, _path(src), obj) if DPP_PASS and name.startswith("lg_inst_") else cmd, keyf, key))

    def run(t):
        name, cmd, keyf, key = t
        if os.path.exists(keyf):
            os.remove(keyf)
        r = _compile_through_pass(name, *cmd[1:]) if cmd[0] == "pass" else subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            with open(keyf, "w") as f:
                f.write(key)
        if verbose:
            print(f"build.py: {name}: rc {r.returncode}", file=sys.stderr)
        return name, r
    err = ""
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        for name, r in ex.map(run, todo):
            if r.returncode != 0 and not err:
                err = f"[{name}] " + r.stderr
    return objs, err


_PASS_FALLBACK = False      # set by build(allow_fallback=True)


class _Result:
    def __init__(self, returncode, stderr):
        self.returncode, self.stderr = returncode, stderr


def _compile_through_pass(name, base, src, obj):
    """hipcc -S (device) -> dpp_hazard_pass -> assembler -> lld -> offload bundle -> host compile embedding the bundle (module doc)."""
    sys.path.insert(0, HERE)
    import dpp_hazard_pass
    stem = os.path.join(OBJ, name)
    steps = [[*base, "--cuda-device-only", "-S", "-o", stem + ".s", src]]
    r = subprocess.run(steps[0], capture_output=True, text=True)
    if r.returncode != 0:
        return r
    try:
        with open(stem + ".s") as f:
            text, stats = dpp_hazard_pass.fix(f.read(), mode=PASS_MODE)
        left = dpp_hazard_pass.check(text, mode=PASS_MODE)
    except dpp_hazard_pass.PassError as e:
        return _Result(1, str(e))
    if left:
        return _Result(1, f"dpp_hazard_pass: {len(left)} unresolved DPP hazard(s), first: {left[0]}")
    with open(stem + ".fix.s", "w") as f:
        f.write(text)
    with open(stem + ".pass.json", "w") as f:
        json.dump(stats, f)
    for cmd in ([os.path.join(LLVM_BIN, "clang"), "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", stem + ".fix.s", "-o", stem + ".dev.o"],
                [os.path.join(LLVM_BIN, "lld"), "-flavor", "gnu", "-m", "elf64_amdgpu", "--no-undefined", "-shared", stem + ".dev.o", "-o", stem + ".co"],
                [os.path.join(LLVM_BIN, "clang-offload-bundler"), "-type=o", "-bundle-align=4096",
                 "-targets=host-x86_64-unknown-linux-gnu,hipv4-amdgcn-amd-amdhsa--gfx950", "-input=/dev/null", "-input=" + stem + ".co", "-output=" + stem + ".hipfb"],
                [*base, "--cuda-host-only", "-Xclang", "-fcuda-include-gpubinary", "-Xclang", stem + ".hipfb", "-c", src, "-o", obj]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            err = " ".join(cmd[:3]) + " ...: " + r.stderr
            if not _PASS_FALLBACK:
                return _Result(r.returncode, err)
            # the driver hook may not fail on tooling around the compiler: plain `hipcc -c` (every marked nop stays), on record
            print(f"build.py: {name}: assembly pipeline failed, compiled with plain hipcc -c instead: {err[-300:]}", file=sys.stderr)
            with open(stem + ".pass.json", "w") as f:
                json.dump({"pipeline_failed": 1}, f)
            return subprocess.run([*base, "-c", src, "-o", obj], capture_output=True, text=True)
    for ext in (".s", ".dev.o", ".co", ".hipfb"):      # .fix.s stays next to the object: it is what tools/isa_loop_stats.py reads
        try:
            os.remove(stem + ext)
        except OSError:
            pass
    return _Result(0, "")


def pass_stats():
    """Sum of the hazard pass's counters over the kernel groups of the last build (None when it did not run)."""
    tot = None
    for g in range(N_GROUPS):
        try:
            with open(os.path.join(OBJ, f"lg_inst_{g}.pass.json")) as f:
                st = json.load(f)
        except (OSError, ValueError):
            continue
        tot = tot or {}
        for k, v in st.items():
            tot[k] = tot.get(k, 0) + v
    return tot


def build(force=False, verbose=False, allow_fallback=None, jobs=None):
    """Compile csrc/liblgsim.so.  The flags actually used are written next to it (liblgsim.build.json) and echoed by bench.py
    in its JSON line, so the scheduling strategy of a measured binary is on record.

    The iterative-ilp scheduler has crashed clang (SIGSEGV in the register allocator) on some shapes of this kernel during
    development.  By default such a failure FAILS the build.  `allow_fallback=True` (or LG_ALLOW_FLAG_FALLBACK=1; the driver
    hook __graft_entry__.build() opts in) retries with the max-ilp strategy and then the default scheduler (within ~1 % / ~3 %
    on the bench) and records `"fallback": true` plus the compiler's error in the sidecar."""
    if not force and not needs_build():
        return OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if allow_fallback is None:
        allow_fallback = os.environ.get("LG_ALLOW_FLAG_FALLBACK", "0") == "1"
    global _PASS_FALLBACK
    _PASS_FALLBACK = bool(allow_fallback)
    if jobs is None:
        jobs = int(os.environ.get("LG_BUILD_JOBS", str(min(8, os.cpu_count() or 1))))
    attempts = [EXTRA_FLAGS]
    if allow_fallback and "LG_HIPCC_FLAGS" not in os.environ:
        attempts += FALLBACK_FLAGS
    first_err, done = "", False
    for flags in attempts:
        objs, err = _compile_all(hipcc, flags, force, jobs, verbose)
        if not err:
            r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT, *objs], capture_output=True, text=True)
            err = r.stderr if r.returncode != 0 else ""
        if not err:
            fell = flags is not attempts[0]
            if fell:
                print("build.py: primary flags failed, compiled with FALLBACK flags " + " ".join(flags), file=sys.stderr)
            ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.splitlines()
            with open(SIDECAR, "w") as f:
                json.dump({"flags": ["--offload-arch=gfx950", "-O3", *flags], "fallback": fell,
                           "primary_flags": EXTRA_FLAGS, "primary_error": first_err[-1500:] if fell else "",
                           "hipcc": next((l for l in ver if "HIP version" in l), ver[0] if ver else ""),
                           "source_hash": source_hash(), "translation_units": len(objs),
                           "dpp_hazard_pass": pass_stats() if DPP_PASS else None,
                           "dpp_pass_mode": PASS_MODE if DPP_PASS else None}, f, indent=1)
            done = True
            break
        first_err = first_err or err
    if not done:
        raise RuntimeError("hipcc failed" + ("" if allow_fallback else " (no flag fallback: set LG_ALLOW_FLAG_FALLBACK=1 to retry with the "
                           "max-ilp / default scheduler)") + ":\n" + first_err[-4000:])
    return OUT


if __name__ == "__main__":
    import time
    t0 = time.time()
    print(build(force="--force" in sys.argv, verbose=True), f"{time.time() - t0:.0f} s")
