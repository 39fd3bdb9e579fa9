"""Pin the committed constant tables (dav1d-mirror_amd/csrc/dsp_tables.h) to
the reference's own data, src/tables.c.

Every kernel, the C oracle and both numpy restatements read
csrc/dsp_tables.h, which tools/gen_tables.py extracted with regular
expressions; an extraction slip (the filter-intra [5][64] -> [5][8][7]
re-layout, the x86-vs-C tap order of src/tables.c:746-758, a dropped zero of
the sparse dr_intra_derivative) would pass every other test.  This test
parses tables.c by a different method: it cuts each table's definition out
of the file as whole lines (no value parsing in Python) and lets the C
compiler evaluate the initialisers (designated initialisers, the F() macro of
the filter-intra table, sparse zeros), once with ARCH_X86 = 0 and once with
ARCH_X86 = 1, next to the committed header's values.

The suite carries no copy of tables.c.  `python tests/test_cpu_tables_pin.py
REFERENCE_DIR` does the cutting and compiling against a dav1d 1.4.1 tree and
records, per table and per ARCH_X86, the element count and the SHA-256 of
the elements printed in the reference's order (tests/golden/tables_pin.json:
digests only, no table data).  The test prints the committed header's
elements through the same program text in the same order and compares count
and digest, so every element of every table is still pinned, in both
layouts, with nothing outside the repository read at test time; on a
mismatch the recording command above names the element when it is run with
--compare.

Tables (src/tables.c line of the definition): dav1d_sgr_params :415,
dav1d_sgr_x_by_x :422, dav1d_mc_subpel_filters :443, dav1d_mc_warp_filter
:547, dav1d_resize_filter :651, dav1d_sm_weights :686,
dav1d_dr_intra_derivative :714, dav1d_filter_intra_taps :759,
dav1d_obmc_masks :808, dav1d_gaussian_sequence :825; and the batch kernel's
packed banks dspt_mc8 / dspt_mc16 derived from the sub-pel filters (m = 0
the identity tap).
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tables_pin.json")
N_ELEMENTS = 32 + 256 + 720 + 96 * 6 + 1544 + 512 + 128 + 44 + 280 + 64 + 2048

NAMES = ("dav1d_sgr_params", "dav1d_sgr_x_by_x", "dav1d_mc_subpel_filters", "dav1d_mc_warp_filter",
         "dav1d_resize_filter", "dav1d_sm_weights", "dav1d_dr_intra_derivative", "dav1d_filter_intra_taps",
         "dav1d_obmc_masks", "dav1d_gaussian_sequence")


def _cut(lines, name):
    """The definition of `name` as whole lines: from its `const` line to the
    first line that closes it (`};`)."""
    start = next(i for i, l in enumerate(lines) if l.startswith("const ") and re.search(r"\b%s\b" % name, l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip() == "};")
    return lines[start:end + 1]


def _f_macro(lines):
    """The `#if ARCH_X86 ... #endif` block that defines F() for the
    filter-intra table."""
    i = next(i for i, l in enumerate(lines) if "dav1d_filter_intra_taps" in l)
    start = max(j for j in range(i) if lines[j].startswith("#if ARCH_X86"))
    end = next(j for j in range(start, i) if lines[j].startswith("#endif"))
    return lines[start:end + 1]


# One program text for both sides: E(header element, tables.c element) prints
# the header's element, or with -DSIDE_REF the reference's, one table a line.
_DUMP = r"""
#include <stdio.h>
#ifdef SIDE_REF
#define E(got, want) printf(" %ld", (long)(want))
#else
#define DSPT_QUAL static const
#include "dsp_tables.h"
#define E(got, want) printf(" %ld", (long)(got))
#endif
#define TABLE(name) printf("%s%s", first ? "" : "\n", name), first = 0

int main(void) {
    int first = 1;
    TABLE("sgr_params");
    for (int i = 0; i < 16; i++) for (int k = 0; k < 2; k++)
        E(dspt_sgr_params[2 * i + k], dav1d_sgr_params[i][k]);
    TABLE("sgr_x_by_x");
    for (int i = 0; i < 256; i++) E(dspt_sgr_x_by_x[i], dav1d_sgr_x_by_x[i]);
    TABLE("subpel");
    for (int b = 0; b < 6; b++) for (int m = 0; m < 15; m++) for (int t = 0; t < 8; t++)
        E(dspt_subpel[(b * 15 + m) * 8 + t], dav1d_mc_subpel_filters[b][m][t]);
    TABLE("mc8_mc16");
    for (int b = 0; b < 6; b++) for (int m = 0; m < 16; m++) {
#ifdef SIDE_REF
        signed char tap[8];
        for (int t = 0; t < 8; t++) tap[t] = m ? dav1d_mc_subpel_filters[b][m - 1][t] : (t == 3 ? 64 : 0);
#endif
        for (int i = 0; i < 2; i++) {
#ifdef SIDE_REF
            unsigned v = 0;
            for (int j = 0; j < 4; j++) v |= (unsigned)(unsigned char)tap[4 * i + j] << (8 * j);
#endif
            E(dspt_mc8[(b * 16 + m) * 2 + i], v);
        }
        for (int i = 0; i < 4; i++) {
#ifdef SIDE_REF
            unsigned v = (unsigned)(unsigned short)tap[2 * i] | (unsigned)(unsigned short)tap[2 * i + 1] << 16;
#endif
            E(dspt_mc16[(b * 16 + m) * 4 + i], v);
        }
    }
    TABLE("warp");
    for (int r = 0; r < 193; r++) for (int t = 0; t < 8; t++)
        E(dspt_warp[r * 8 + t], dav1d_mc_warp_filter[r][t]);
    TABLE("resize");
    for (int r = 0; r < 64; r++) for (int t = 0; t < 8; t++)
        E(dspt_resize[r * 8 + t], dav1d_resize_filter[r][t]);
    TABLE("sm_weights");
    for (int i = 0; i < 128; i++) E(dspt_sm_weights[i], dav1d_sm_weights[i]);
    TABLE("dr_deriv");
    for (int i = 0; i < 44; i++) E(dspt_dr_deriv[i], dav1d_dr_intra_derivative[i]);
    /* the header's [filter][output idx][tap k] against the reference's flat
       [filter][64] in the layout ARCH_X86 selects */
    TABLE("filter_intra");
    for (int f = 0; f < 5; f++) for (int idx = 0; idx < 8; idx++) for (int k = 0; k < 7; k++) {
        const int pos = ARCH_X86 ? 2 * idx + 16 * (k >> 1) + (k & 1) : idx + 8 * k;
        (void)pos;
        E(dspt_filter_intra[(f * 8 + idx) * 7 + k], dav1d_filter_intra_taps[f][pos]);
    }
    TABLE("obmc");
    for (int i = 0; i < 64; i++) E(dspt_obmc[i], dav1d_obmc_masks[i]);
    TABLE("gaussian");
    for (int i = 0; i < 2048; i++) E(dspt_gaussian[i], dav1d_gaussian_sequence[i]);
    printf("\n");
    return 0;
}
"""


def _run(workdir, tag, body, flags):
    """Compile body + _DUMP, run it, return {table: [elements as text]}."""
    src = os.path.join(workdir, f"pin_{tag}.c")
    with open(src, "w") as f:
        f.write("\n".join(body) + "\n" + _DUMP)
    exe = os.path.join(workdir, f"pin_{tag}")
    subprocess.run(["cc", "-std=c11", "-O0", "-Werror=override-init"] + flags + [src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, check=True)
    return {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l.strip()}


def header_tables(workdir, x86):
    return _run(workdir, f"hdr{x86}", [f"#define ARCH_X86 {x86}"],
                ["-I", os.path.join(ROOT, "dav1d-mirror_amd", "csrc")])


def reference_tables(workdir, ref, x86):
    """The same dump of a dav1d tree's src/tables.c, its definitions cut out
    as whole lines and evaluated by the C compiler."""
    lines = open(os.path.join(ref, "src", "tables.c")).read().splitlines()
    body = ["#include <stdint.h>", "#include <dav1d/headers.h>", "#define ALIGN(decl, a) decl",
            f"#define ARCH_X86 {x86}", "#define SIDE_REF 1"]
    for name in NAMES:
        if name == "dav1d_filter_intra_taps":
            body += _f_macro(lines)
        body += _cut(lines, name)
    return _run(workdir, f"ref{x86}", body, ["-I", os.path.join(ref, "include")])


def digests(tables):
    return {k: {"n": len(v), "sha256": hashlib.sha256(" ".join(v).encode()).hexdigest()} for k, v in tables.items()}


@pytest.mark.parametrize("x86", [0, 1])
def test_tables_match_reference(tmp_path, x86):
    want = json.load(open(GOLDEN))[f"arch_x86_{x86}"]
    got = digests(header_tables(str(tmp_path), x86))
    assert sorted(got) == sorted(want)
    assert sum(v["n"] for v in want.values()) == N_ELEMENTS
    for name in want:
        assert got[name] == want[name], f"{name}: dsp_tables.h differs from the recorded src/tables.c"


if __name__ == "__main__":
    import tempfile
    ref = [a for a in sys.argv[1:] if not a.startswith("--")][0]
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for x in (0, 1):
            rt = reference_tables(d, ref, x)
            out[f"arch_x86_{x}"] = digests(rt)
            if "--compare" in sys.argv:
                ht = header_tables(d, x)
                for k in rt:
                    bad = [i for i, (a, b) in enumerate(zip(ht[k], rt[k])) if a != b]
                    print(f"ARCH_X86={x} {k}: header {len(ht[k])} elements, tables.c {len(rt[k])}, "
                          + (f"first mismatch [{bad[0]}]: header {ht[k][bad[0]]}, tables.c {rt[k][bad[0]]}"
                             if bad else "equal"))
    if "--compare" not in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
