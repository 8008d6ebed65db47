#!/usr/bin/env python3
# isa_table.py A.s B.s: per kernel of two `hipcc --offload-device-only -S` files, A/B resource metadata and instruction counts, and
# whether the opcode sequence (operands ignored) from the first to the last v_mfma is the same.
import re, sys
KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")
OPS = ("v_mfma", "ds_read", "global_load", "global_store", "buffer_", "s_barrier", "")
def kernels(text, out={}):
    for name, body in re.findall(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):  # (a kernel can hold several s_endpgm)
        ops = [l.split()[0] for l in body.splitlines() if l.startswith("\t") and l.lstrip()[0] not in ";."]
        m = [i for i, o in enumerate(ops) if o.startswith("v_mfma")] or [0]
        meta = re.search(r"^  - \.agpr_count((?!^  - ).)*?^    \.name: +%s\n.*?^    \.wavefront_size" % name, text, re.M | re.S).group(0)
        out[name] = [re.search(r"^    \.%s: +(\d+)" % k, meta, re.M).group(1) for k in KEYS] + [sum(o.startswith(p) for o in ops) for p in OPS] + [ops[m[0]:m[-1] + 1]]
    return dict(out)
a, b = (kernels(open(f).read(), {}) for f in sys.argv[1:3])
print(" | ".join(("kernel",) + KEYS + OPS[:-1] + ("instructions", "mfma span")))
for k in sorted(a):
    print(" | ".join([k] + ["%s/%s" % xy for xy in zip(a[k][:-1], b[k][:-1])] + ["same" if a[k][-1] == b[k][-1] else "DIFFERENT"]))
