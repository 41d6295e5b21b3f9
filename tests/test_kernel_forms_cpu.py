"""No GPU: the ownership table of tests/kernel_forms.py names kernels and owners that exist.  A renamed kernel, check or test
must take its entries along -- otherwise the table would own instances that no launch can produce, or point at nothing."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lm_net_amd", "csrc")


def _launched_kernels():
    """Base names of every kernel that reaches LMN_LAUNCH: its first argument, and for a launcher macro that passes one of its own
    parameters on (LMN_WDK(KERN, ...)) the kernel names pasted where the macro is used."""
    texts = [open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))]
    first = re.compile(r"LMN_LAUNCH\(\s*\(?\s*([A-Za-z_]\w*)")
    found = set()
    for t in texts:
        found |= set(first.findall(t))
    for t in texts:
        for m in re.finditer(r"#define\s+(\w+)\(([^)]*)\)((?:[^\n]*\\\n)*[^\n]*)", t):
            macro, params, body = m.group(1), [p.strip() for p in m.group(2).split(",")], m.group(3)
            for idx, p in enumerate(params):
                if p and p in first.findall(body):
                    for t2 in texts:
                        for use in re.finditer(r"(?<!define )\b%s\(([^;]*?)\)\s*;" % re.escape(macro), t2):
                            args = [a.strip() for a in use.group(1).split(",")]
                            if idx < len(args) and re.fullmatch(r"[a-z_]\w*", args[idx]):
                                found.add(args[idx])
    return found


def _functions(path):
    return {n.name for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.FunctionDef)}


def test_owned_kernels_are_launched_somewhere():
    import kernel_forms
    kernels = _launched_kernels()
    assert "wgrad_1x1w_kernel" in kernels and "conv_pack_kernel" in kernels and "det_sum_kernel" in kernels   # (the parser sees plain, templated and macro-pasted launches)
    missing = sorted({k for k in kernel_forms.OWNED if k.split("<")[0] not in kernels})
    assert not missing, "OWNED names kernels that no LMN_LAUNCH in lm_net_amd/csrc launches: %s" % missing


def test_owners_exist():
    import kernel_forms
    # (kernel_checks.py with its driver test_kernels_gpu.py; kernel_checks_envelope.py with test_kernels_envelope_gpu.py)
    homes = [(_functions(os.path.join(ROOT, "tests", c)), open(os.path.join(ROOT, "tests", t)).read())
             for c, t in (("kernel_checks.py", "test_kernels_gpu.py"), ("kernel_checks_envelope.py", "test_kernels_envelope_gpu.py"))]
    bad = []
    for owner in sorted(set(kernel_forms.OWNED.values())):
        if "::" in owner:
            path, test = owner.split("::", 1)
            full = os.path.join(ROOT, path)
            if not (path.startswith("tests/") and os.path.isfile(full) and test.split("[")[0] in _functions(full)):
                bad.append(owner)
        elif not (owner.startswith("check_") and any(owner in checks and '"%s"' % owner in listed for checks, listed in homes)):
            bad.append(owner)
    assert not bad, "owners that are neither a check_* run by its driver test nor an existing test: %s" % bad


def test_owned_by_partitions_the_table():
    import kernel_forms
    assert kernel_forms.OWNED, "empty ownership table"
    total = sum(len(kernel_forms.owned_by(o)) for o in set(kernel_forms.OWNED.values()))
    assert total == len(kernel_forms.OWNED)
    assert kernel_forms.owned_by("check_no_such_check") == set()
