#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device assemblies of one source file: do the kernels of A compile to the same instructions
in B?  Comments and the function number inside basic-block labels are ignored (they shift when kernels are added to the file);
everything else — instructions, operands, directives, the kernel descriptors' values — must be equal.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -S --cuda-device-only \\
          -Rpass-analysis=kernel-resource-usage csrc/input_form_kernels.hip -o new.s 2> new_usage.txt      (and the parent's)
    python tools/isa_ab.py parent.s new.s

For kernels that moved between files, concatenate the .s files of either side (as for profiles/kernel_files_split_isa_ab.txt).
"""
import hashlib
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                out[name], name = body, None
            else:
                text = re.sub(r"\s+", " ", re.sub(r"BB\d+_", "BB_", line.split(";")[0])).strip()
                if text:
                    body.append(text)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    differ = 0
    for k, body in a.items():
        same = b.get(k) == body
        differ += not same
        n = sum(1 for t in body if not t.startswith(".") and not t.endswith(":"))
        print(f"{k[:70]:70s} {n:6d} instructions  sha256 {hashlib.sha256(chr(10).join(body).encode()).hexdigest()[:16]}  "
              f"{'identical' if same else 'DIFFERS' if k in b else 'MISSING'}")
    for k in b:
        if k not in a:
            print(f"{k[:70]:70s} new")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
