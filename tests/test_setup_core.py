"""The host arithmetic of a run's setup (addapt_amd/csrc/setup_core.hpp) without a GPU: a
stand-alone program built against the header and energy.cpp alone prints what the core
builds, and every value is compared with a restatement on numpy arrays or with a case
derived by hand -- never with the core itself.  The program is built once more with the
address and undefined-behaviour sanitizers (stand-alone: nothing is preloaded).

The one-ulp bound of the partition-function tables is derived, not measured: an entry is
float32(exp(-e * 10 / kT) * sigma^k) of an exact integer energy e, computed in FP64 on
both sides, so the only freedom is libm's last double bit before the rounding to float.

An odd cycle (move error 3) needs three macrostates: two macrostates are two matchings,
and the union of two matchings closes even cycles only."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "addapt_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "setup_core_probe.cc")
PAR = os.path.join(ROOT, "addapt_amd", "data", "rna_turner2004_addapt.par")
MFE_BIG = 1.0e7
G0 = -0.30
# dev_types.hpp: offsets into DevScaled::ctab, the generic interior rows
CT_STK, CT_FB, CT_F1N, FG_ROW = 800, 864, 896, 27
# DevTables: float counts of its members, in order
TABLES = [("stack", 64), ("mmH", 200), ("mmI", 200), ("mm1n", 200), ("mm23", 200), ("mlstem", 200), ("ext", 288),
          ("termAU", 8), ("int11", 1600), ("int21", 8000), ("int22", 40000)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    out = str(tmp_path_factory.mktemp("setup_core") / ("probe" + "_san" * bool(flags)))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", out, SRC,
                    os.path.join(CSRC, "energy.cpp")], check=True)
    return out


def _run(exe, *args, binary=False):
    r = subprocess.run([exe, *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, (args, r.returncode, r.stderr)
    return r.stdout if binary else r.stdout.decode().split("\n")


def _ints(line):
    return [int(x) for x in line.split()]


# ---------------------------------------------------------------- build_constraint
def _constraint(cst, N):
    """(status, message, arrays): the five byte arrays of N + 2 (up, dn, partner, enclosing, flags) of a
    dot-bracket constraint, 1-based with a zero at both ends; "" constrains nothing."""
    c = cst or "." * N
    partner, enc, flg = (np.zeros(N + 2, dtype=np.int64) for _ in range(3))
    stack = []
    for i in range(1, N + 1):
        enc[i] = stack[-1] if stack else 0
        if c[i - 1] == "(":
            stack.append(i)
        elif c[i - 1] == ")":
            if not stack:
                return 3, "unbalanced ')' in constraint '%s'" % cst, None
            a = stack.pop()
            partner[a], partner[i] = i, a
            enc[i] = stack[-1] if stack else 0
    if stack:
        return 3, "unbalanced '(' in constraint '%s'" % cst, None
    for i in range(1, N + 1):
        flg[i] = {"x": 1, "<": 2, ">": 4, "|": 8}.get(c[i - 1], 0)
    free = np.array([0] + [int(c[i - 1] not in "|<>" and partner[i] == 0) for i in range(1, N + 1)] + [0])
    up, dn = np.zeros(N + 2, dtype=np.int64), np.zeros(N + 2, dtype=np.int64)
    for i in range(N, 0, -1):      # unconstrained positions from i on ...
        up[i] = up[i + 1] + 1 if free[i] else 0
    for i in range(1, N + 1):      # ... and up to i
        dn[i] = dn[i - 1] + 1 if free[i] else 0
    return 0, "", np.stack([np.minimum(up, 255), np.minimum(dn, 255), partner, enc, flg])


@pytest.mark.parametrize("cst,N", [("", 12), ("((((....))))", 12), ("..((xx|<>..))..", 15), ("(()", 3), ("())", 3),
                                   ("(x(", 3), ("." * 255, 255)])
def test_build_constraint(exe, cst, N):
    status, msg, ref = _constraint(cst, N)
    out = _run(exe, "constraint", N, cst)
    assert (int(out[0]), out[1]) == (status, msg)
    if status:
        assert cst in ("(()", "())", "(x(") and status == 3   # ADX_ECONSTRAINT
        return
    got = np.array([_ints(l) for l in out[2:7]])
    assert got.shape == (5, N + 2)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    if N == 255:   # the run lengths reach the byte's limit at the ends
        assert got[0][1] == 255 and got[1][255] == 255 and got[0][255] == 1


# ---------------------------------------------------------------- closure
TEMPLATE, HAIRPIN = "ACGUACGUACGU", "((((....))))"
MOVE_TEXT = {1: "mismatched base-pair in macrostate",
             2: "position can be mutated, but it's base-paired to a position which can't be",
             3: "no way to satisfy all base pairing constraints."}


def test_closure_of_a_hairpin(exe):
    for pos in range(12):
        out = _run(exe, "closure", TEMPLATE, pos, HAIRPIN)
        pairs = [tuple(_ints(l)) for l in out[2:] if l]
        assert out[0] == "0"
        if HAIRPIN[pos] == ".":
            assert pairs == [(pos, 0)]
        else:
            assert pairs == [(pos, 0), (11 - pos, 1)]   # the hairpin pairs k with 11 - k


@pytest.mark.parametrize("code,seq,pos,macs", [
    (1, "AAA", 0, ["(.."]),                   # the bracket never closes
    (2, "AAa", 0, ["(.)"]),                   # the partner is lower case: not mutable
    (3, "AAA", 0, ["(.)", ".()", "()."])])    # 0-2, 2-1, 1-0: position 0 would need both parities
def test_closure_errors(exe, code, seq, pos, macs):
    out = _run(exe, "closure", seq, pos, *macs)
    assert int(out[0]) == code and out[1] == MOVE_TEXT[code]


# ---------------------------------------------------------------- build_tables / build_scaled
def _ulps(got, ref):
    """FP32 steps between two arrays of non-negative floats"""
    g, r = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert (g >= 0).all() and (r >= 0).all()
    return np.abs(g.view(np.int32).astype(np.int64) - r.view(np.int32).astype(np.int64))


def _factor(e_mfe, kT, sigma=1.0, k=0):
    """What the PF tables hold where the MFE tables hold e_mfe (dcal, or MFE_BIG), in FP64 rounded to FP32"""
    e = np.asarray(e_mfe, dtype=np.float64)
    big = e == MFE_BIG
    assert (e[~big] == np.floor(e[~big])).all() and (np.abs(e[~big]) < 1e5).all()   # exact integer energies
    f = np.exp(-np.where(big, 0.0, e) * 10.0 / kT) * np.power(sigma, np.asarray(k, dtype=np.float64))
    return np.where(big, 0.0, f).astype(np.float32)


@pytest.fixture(scope="module")
def kT(exe):
    v = float(_run(exe, "kt")[0])
    assert abs(v - (37.0 + 273.15) * 1.98717) < 1e-9
    return v


def test_build_tables_pf_against_mfe(exe, kT):
    pf = np.frombuffer(_run(exe, "tables", PAR, "pf", binary=True), dtype=np.float32)
    mfe = np.frombuffer(_run(exe, "tables", PAR, "mfe", binary=True), dtype=np.float32)
    assert pf.size == mfe.size == sum(n for _, n in TABLES)
    worst = _ulps(pf, _factor(mfe, kT))
    print("DevTables: %d floats, %d possible, worst %d ulp" % (pf.size, int((mfe != MFE_BIG).sum()), worst.max()))
    assert worst.max() <= 1
    o = 0
    for name, n in TABLES:   # every member holds energies, and pair type 0 is impossible
        assert (mfe[o:o + n] != MFE_BIG).any(), name
        o += n
    assert (mfe[:8] == MFE_BIG).all() and (pf[:8] == 0).all()


def _scaled(exe, mode):
    out = {}
    for l in _run(exe, "scaled", PAR, mode, G0):
        if l:
            name, *vals = l.split()
            out[name] = np.array([float(v) for v in vals])
    return out


@pytest.fixture(scope="module")
def scaled(exe):
    return _scaled(exe, "pf"), _scaled(exe, "mfe")


def test_build_scaled_pf_against_mfe(scaled, kT):
    pf, mfe = scaled
    sigma = np.exp(G0 / (kT / 1000.0))
    u32, u31 = np.arange(32), np.arange(31)
    fg_u = 6 + np.arange(25 * FG_ROW) // FG_ROW
    cases = [("ctab stack", pf["ctab"][CT_STK:CT_STK + 64], mfe["ctab"][CT_STK:CT_STK + 64], 0),
             ("ctab bulge", pf["ctab"][CT_FB:CT_FB + 32], mfe["ctab"][CT_FB:CT_FB + 32], u32 + 2),
             ("ctab 1 x n", pf["ctab"][CT_F1N:CT_F1N + 32], mfe["ctab"][CT_F1N:CT_F1N + 32], u32 + 3),
             ("fgen", pf["fgen"], mfe["fgen"], fg_u + 2),
             ("hp", pf["hp"][:31], mfe["hp"][:31], u31 + 2),
             ("sig", pf["sig"], mfe["sig"], np.arange(pf["sig"].size)),
             ("mlclosing", pf["mlclosing"], mfe["mlclosing"], 2)]
    for name, got, e, k in cases:
        worst = _ulps(got, _factor(e, kT, sigma, k))
        print("%s: %d values, %d possible, worst %d ulp" % (name, got.size, int((e != MFE_BIG).sum()), worst.max()))
        assert worst.max() <= 1, name
        assert (got > 0).any(), name
    assert (mfe["sig"] == 0).all()   # an energy carries no scale


@pytest.mark.parametrize("mode", [0, 1])
def test_term_lists(scaled, mode):
    X = scaled[mode]
    s_cnt, g_cnt = X["s_cnt"].astype(int), X["g_cnt"].astype(int)
    assert (np.diff(s_cnt) >= 0).all() and (np.diff(g_cnt) >= 0).all()
    assert s_cnt[31] == s_cnt[30] and g_cnt[31] == g_cnt[30]
    seen = {}
    for t in range(s_cnt[30]):
        n1, n2 = int(X["s_n1"][t]), int(X["s_n2"][t])
        seen[(n1, n2)] = seen.get((n1, n2), 0) + 1
        assert s_cnt[n1 + n2 - 1] <= t < s_cnt[n1 + n2] if n1 + n2 else t < s_cnt[0]   # ordered by loop size
    for t in range(g_cnt[30]):
        n1, u = int(X["g_n1"][t]), int(X["g_u"][t])
        seen[(n1, u - n1)] = seen.get((n1, u - n1), 0) + 1
        assert g_cnt[u - 1] <= t < g_cnt[u]
    want = {(n1, u - n1) for u in range(31) for n1 in range(u + 1)}
    assert set(seen) == want and set(seen.values()) == {1}


# ---------------------------------------------------------------- pack16
def test_pack16(exe):
    fits = [-16383, 16383, 0]
    out = _run(exe, "pack16", *fits, MFE_BIG, MFE_BIG / 2, -16384, 16384, 0.5)
    for v, l in zip(fits, out):
        h = v & 0xFFFF
        assert l == "1 %08x" % (h | h << 16)
    assert out[3] == out[4] == "1 7fff7fff"
    assert out[5:8] == ["0", "0", "0"]


# ---------------------------------------------------------------- groups2 and the outside slots
def test_groups2_pairs_apo_with_holo(exe):
    # (context, macrostate, N, holo): ctx 0 apo, ctx 0 holo, ctx 0 mac 0 apo, ctx 0 mac 0 holo, ctx 1 apo
    out = _run(exe, "groups", "0,-1,40,0", "0,-1,40,1", "0,0,40,0", "0,0,40,1", "1,-1,44,0")
    assert _ints(out[0]) == [0, 1, 2, 3, 4, 4]


def test_outside_slots(exe):
    out = _run(exe, "slots", "0,1,2,3,4,4", "1,4,2")
    assert out[0] == "0" and _ints(out[2]) == [1, 4, 2]   # each one's first place in the list
    out = _run(exe, "slots", "0,1,2,3,4,4", "1,5")
    assert (int(out[0]), out[1]) == (1, "internal: outside variant 5 has no fold group")   # ADX_EINVAL
