"""What the host files of the train passes (tests/test_train_host.py, tests/test_train_ee_host.py, tests/test_train_ts_host.py) share, in
one copy: the probe of a header's struct layout and constants, the check of a header's exports and translation unit, the mutations and
the driver of the entry points' refusal tables, and the restated optimizer step.  No test functions here; nothing is launched."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from hcr_genesis_lr_cl_amd import abi
from tests import optim_cases as oc


def check_layout(header, structs, consts):
    """sizeof and every offsetof of the (C name, ctypes class) pairs and the value of every constant (C name -> mirror), as a C compiler
    reads them from the header."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void){"]
    for cname, cls in structs:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += [f'printf("{k} %ld\\n", (long)({k}));' for k in consts] + ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.run(["gcc", "-o", exe, src], check=True)
        got = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for cname, cls in structs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    for k, v in consts.items():
        assert int(got[k]) == v, k


def check_exports(header, exports, unit, includes):
    """The header declares exactly `exports`, the built library has them, and the build compiles `unit`.hip as a translation unit of that
    name which depends on the header and on every file of `includes`.  Returns the declared names."""
    declared = set(re.findall(r"\b(lg_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)))
    assert declared == set(exports)
    lib = C.CDLL(abi.lib_path())
    for sym in declared:
        assert hasattr(lib, sym), sym
    from hcr_genesis_lr_cl_amd import build
    assert any(u[0] == unit and u[1] == unit + ".hip" and any(d.endswith(os.path.basename(header)) for d in u[3]) and all(i in u[3] for i in includes)
               for u in build.units())
    assert unit + ".hip" in build.__doc__
    return declared


def set_path(path, value):
    """A mutation of a descriptor: the member at `path` (attribute names and array indices) set to `value`."""
    def f(a):
        obj = a
        *head, last = path
        for p in head:
            obj = obj[p] if isinstance(p, int) else getattr(obj, p)
        setattr(obj, last, value)
    return f


def refuse(table, i, good, prefix, plan_cls):
    """Row i of a table of (mutation, message, which entry points refuse it: p plan, f forward, b backward): each of those entry points of
    `prefix` returns non-zero on the mutated good() descriptor with the message behind its own name; a plan that is not among them still
    succeeds, as it reads the shapes alone."""
    mutate, msg, who = table[i]
    lib = abi.load_lib()
    a = good()
    mutate(a)
    plan = lambda: getattr(lib, prefix + "_plan")(C.byref(a), C.byref(plan_cls()))
    calls = dict(p=(prefix + "_plan", plan), f=(prefix + "_forward", lambda: getattr(lib, prefix + "_forward")(C.byref(a), None)),
                 b=(prefix + "_backward", lambda: getattr(lib, prefix + "_backward")(C.byref(a), None)))
    for key in who:
        name, call = calls[key]
        assert call() != 0, name
        err = lib.lg_last_error()
        assert err.startswith(name.encode() + b": ") and msg in err, (name, err)
    if "p" not in who:
        assert plan() == 0


def adam(params, grads, state, lr, cfg, kl=None):
    """One restated optimizer step (tests/optim_cases.restate) on a list of arrays; `state` carries the moments and the step count."""
    r = oc.restate(params, [grads], lr0=lr, kls=None if kl is None else [kl], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"],
                   max_grad_norm=cfg["max_grad_norm"], desired_kl=cfg["desired_kl"], exp_avg=state.get("m"), exp_avg_sq=state.get("v"),
                   step0=state.get("step", 0))[0]
    state.update(m=r["exp_avg"], v=r["exp_avg_sq"], step=r["step"])
    return r
