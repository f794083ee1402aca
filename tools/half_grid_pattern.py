#!/usr/bin/env python3
"""Which product of the half-grid mean 0.5 * (g_j + g_j+1) a gfx950 listing fuses, per kernel, when g = a1 * d is a product.

   python tools/half_grid_pattern.py listing.s [kernel-name-substring ...]

The listing is what `hipcc --offload-arch=gfx950 -O3 ... --cuda-device-only -S ibs_kernels.hip -DIBS_M=8` writes.  For every
`v_mul_f64 x, y, 0.5` whose y is an fma / fmac of two products the script prints which chunk point went into the fma (F = fused)
and which was rounded by a v_mul_f64 first (R), the chunk point being the LDS offset of the a1 factor in units of 8 bytes,
relative to the lowest one seen in that kernel.  A run of rows is one pass over a lane's chunk (set-up, or the rebuild of s in
assemble()).  Straight-line tracking of the defining instruction of each register pair: good for the unrolled row loops only.
"""
import re
import subprocess
import sys

PAIR = r"(-?\|?v\[\d+:\d+\]\|?)"
RE_FUNC = re.compile(r"^(_Z\w+):")
RE_DS = re.compile(r"^\s*ds_read_b64 (v\[\d+:\d+\]), v\d+(?: offset:(\d+))?")
RE_3 = re.compile(r"^\s*v_fma_f64 (v\[\d+:\d+\]), " + PAIR + ", " + PAIR + ", " + PAIR + r"\s*$")
RE_MAC = re.compile(r"^\s*v_fmac_f64_e32 (v\[\d+:\d+\]), " + PAIR + ", " + PAIR + r"\s*$")
RE_MUL = re.compile(r"^\s*v_mul_f64 (v\[\d+:\d+\]), " + PAIR + ", " + PAIR + r"\s*$")
RE_HALF = re.compile(r"^\s*v_mul_f64 (v\[\d+:\d+\]), (v\[\d+:\d+\]), 0\.5\s*$")
RE_ANYDEF = re.compile(r"^\s*v_\w+ (v\[\d+:\d+\]),")


def a1_offset(defs, x, y):
    """offset of whichever operand is a plain LDS value (the other is the theta0 fold, an fmac chain)"""
    for r in (x, y):
        d = defs.get(r)
        if d and d[0] == "ds":
            return d[1]
    return None


def scan(lines):
    defs, rows = {}, []
    for ln in lines:
        m = RE_HALF.match(ln)
        if m:
            src = defs.get(m.group(2))
            if src and src[0] == "fma":
                ad = src[2]
                if ad and ad[0] == "mul":
                    rows.append((src[1], ad[3]))
            defs[m.group(1)] = ("other",)
            continue
        m = RE_DS.match(ln)
        if m:
            defs[m.group(1)] = ("ds", int(m.group(2) or 0))
            continue
        m = RE_3.match(ln)
        if m:
            defs[m.group(1)] = ("fma", a1_offset(defs, m.group(2), m.group(3)), defs.get(m.group(4)))
            continue
        m = RE_MAC.match(ln)
        if m:
            defs[m.group(1)] = ("fma", a1_offset(defs, m.group(2), m.group(3)), defs.get(m.group(1)))
            continue
        m = RE_MUL.match(ln)
        if m:
            defs[m.group(1)] = ("mul", m.group(2), m.group(3), a1_offset(defs, m.group(2), m.group(3)))
            continue
        m = RE_ANYDEF.match(ln)
        if m:
            defs[m.group(1)] = ("other",)
    return rows


def main():
    path, want = sys.argv[1], sys.argv[2:]
    name, body, out = None, [], {}
    for ln in open(path):
        m = RE_FUNC.match(ln)
        if m:
            if name:
                out[name] = scan(body)
            name, body = m.group(1), []
        else:
            body.append(ln)
    if name:
        out[name] = scan(body)
    for nm, rows in out.items():
        dem = subprocess.run(["c++filt", nm], capture_output=True, text=True).stdout.split("(")[0].replace("void ", "").strip()
        if want and not any(w in dem for w in want):
            continue
        offs = [o for r in rows for o in r if o is not None]
        if not offs:
            continue
        base = min(offs)
        txt = " ".join("F%s/R%s" % tuple("?" if o is None else str((o - base) // 8) for o in r) for r in rows)
        print("%-44s %s" % (dem, txt))


if __name__ == "__main__":
    main()
