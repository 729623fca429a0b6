"""Do two builds of one .hip file hold the same kernels?  Compile both with the flags of rlsolver_amd/build.py plus
`--cuda-device-only -S` and give the two .s files: every kernel's text, from its label to .end_amdhsa_kernel, by mangled name.
The compiler numbers its local labels (.LBB<f>_<n>, .Lfunc_end<f>, .LJTI<f>_<n>) by the ORDER in which it emits functions, which
follows the order of instantiation in the host code: that number <f> is dropped before comparing (and the padding in front of the comments beside such labels), nothing else.

    python tools/kernel_text_diff.py before.s after.s"""
import collections, re, sys


def kernels(path):
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, flags=re.M))
    out, name, buf = {}, None, []
    for line in text.splitlines(keepends=True):
        if name is None and line[:1] == "_" and line.split(":", 1)[0] in names:
            name, buf = line.split(":", 1)[0], []
        if name is not None:
            buf.append(line)
            if line.strip() == ".end_amdhsa_kernel":
                out[name] = re.sub(r"(\.LBB|\bBB|func_begin|func_end|\.LJTI|\.Ltmp)\d+", r"\1", re.sub(r"[ \t]+;", " ;", "".join(buf)))
                name = None
    assert set(out) == names, "a kernel without a label"
    return out


a, b = (kernels(p) for p in sys.argv[1:3])
family = lambda ks: sorted(collections.Counter(re.sub(r"^_ZN3rls\d+(k_[a-z_0-9]+?)(I.*|E.*)$", r"\1", k) for k in ks).items())
print(len(a), "kernels before,", len(b), "after")
print("families before:", family(a))
only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
print("only before:", only_a[:10], "\nonly after:", only_b[:10], "\ntext differs:", differ[:10])
print("IDENTICAL" if not (only_a or only_b or differ) else f"DIFFERENT: {len(only_a)} / {len(only_b)} / {len(differ)}")
sys.exit(1 if only_a or only_b or differ else 0)
