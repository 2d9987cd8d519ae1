#!/usr/bin/env python3
"""sha256 of every kernel body in a hipcc -S --cuda-device-only listing, for comparing the device code of two trees.  The listing is split
per function the way tools/isa_counts.py does; the function's index in local labels (.LBB<n>_, Header=BB<n>_) and the assembler comments
(their column depends on that index's width) are taken out, nothing else.
   python tools/kernel_digest.py listing.s > digests.txt"""
import hashlib
import re
import sys


def main():
    s = open(sys.argv[1]).read()
    parts = re.split(r'\n\t\.type\t(_Z\S+),@function\n', s)
    rows = []
    for i in range(1, len(parts), 2):
        body = parts[i + 1].split('.Lfunc_end')[0]
        body = re.sub(r'[ \t]*;.*', '', body)
        body = re.sub(r'\.LBB\d+_', '.LBB_', body)
        rows.append((parts[i], hashlib.sha256(body.encode()).hexdigest(), len(re.findall(r'\n\t[a-z]', body))))
    for name, h, n in sorted(rows):
        print(h, n, name)


if __name__ == "__main__":
    main()
