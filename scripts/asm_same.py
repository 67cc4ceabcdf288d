#!/usr/bin/env python
"""Do two device-assembly listings (`hipcc ... --cuda-device-only -S`) hold the same code?

  python scripts/asm_same.py before.s after.s [more pairs ...]

hipcc's listing of one unchanged source differs from run to run: the
`__hip_cuid_<hash>` symbol is new in every compilation, and the read-only
tables (`.rodata` objects) come out in varying order.  So a plain diff of two
builds is never empty.  This compares what can be compared: the `__hip_cuid`
hash is masked, the instruction and label stream (everything that is code)
must be identical line for line in order, and all remaining lines must be the
same as a multiset.  Exit status 0 when every pair agrees.
"""

import re
import sys

CODE = re.compile(r"\t(v_|s_|global_|flat_|ds_|buffer_|scratch_)|^[._A-Za-z0-9$]+:")


def load(path):
    return [re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", line) for line in open(path).read().split("\n")]


def main(argv):
    if len(argv) < 2 or len(argv) % 2:
        sys.exit(__doc__)
    bad = 0
    for a, b in zip(argv[::2], argv[1::2]):
        la, lb = load(a), load(b)
        tables = {m.group(1) for line in la + lb for m in [re.match(r"\t\.type\t(\S+),@object", line)] if m}
        code = lambda lines: [x for x in lines if CODE.match(x) and x.rstrip(":") not in tables]  # noqa: E731
        same_code, same_lines = code(la) == code(lb), sorted(la) == sorted(lb)
        print(f"{a} / {b}: code stream {'identical' if same_code else 'DIFFERS'} ({len(code(la))} lines), "
              f"other lines {'the same set' if same_lines else 'DIFFER'}")
        bad += not (same_code and same_lines)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
