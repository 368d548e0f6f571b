// Host arithmetic of a run's setup, which decides what every fold kernel reads:
// energy tables and scaled constants, the ligand motif, constraint blobs, the
// packed 16-bit MFE tables, the apo / holo fold groups, the move closures.
// Plain C++ (no HIP): the API layer uploads what these build and hands a
// SetupError to fail() unchanged; tests/test_setup_core.py checks them stand-alone.
#pragma once

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#ifndef __HIPCC__   // dev_types.hpp marks its inline helpers for both sides
#define __host__
#define __device__
#endif

#include "../../include/addapt_gpu.h"
#include "dev_types.hpp"
#include "energy.hpp"

namespace adx {

struct SetupError {
    adx_status status = ADX_OK;
    std::string text;
};

inline adx_status setup_fail(SetupError &err, adx_status s, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err.status = s;
    err.text = buf;
    return s;
}

inline double boltz_d(double e_dcal) {
    if (e_dcal >= INF_E / 2) return 0.0;
    return std::exp(-e_dcal * 10.0 / kT_cal());
}
inline float boltz(double e_dcal) { return static_cast<float>(boltz_d(e_dcal)); }

// Loop factor of energy e (dcal/mol) spanning k scaled nucleotides: the
// Boltzmann factor exp(-e/kT) sigma^k (partition function) or the energy
// itself (MFE; INF_E and above -> MFE_BIG).  dev_types.hpp "Fold modes".
// FT: the tables' type (dev_types.hpp DevTablesT: float for the engine)
template <class FT>
struct Fac {
    bool mfe;
    double sigma;
    FT operator()(double e, int k = 0) const {
        if (mfe) return e >= INF_E ? FT(MFE_BIG) : static_cast<FT>(e);
        return static_cast<FT>(boltz_d(e) * std::pow(sigma, k));
    }
    FT zero() const { return mfe ? FT(MFE_BIG) : FT(0); }
    FT one() const { return mfe ? FT(0) : FT(1); }
};

template <class FT>
inline void build_tables(const EnergyParams &P, DevTablesT<FT> &T, bool mfe) {
    const Fac<FT> F{mfe, 1.0};
    FT *flat = reinterpret_cast<FT *>(&T);
    for (size_t k = 0; k < sizeof(DevTablesT<FT>) / sizeof(FT); k++) flat[k] = F.zero();
    for (int a = 1; a <= 7; a++) {
        for (int b = 1; b <= 7; b++) T.stack[a][b] = F(P.stack[a][b]);
        for (int x = 0; x < 5; x++)
            for (int y = 0; y < 5; y++) {
                T.mmH[a][x][y] = F(P.mmH[a][x][y]);
                T.mmI[a][x][y] = F(P.mmI[a][x][y]);
                T.mm1n[a][x][y] = F(P.mm1nI[a][x][y]);
                T.mm23[a][x][y] = F(P.mm23I[a][x][y]);
                T.mlstem[a][x][y] = F(ml_stem_energy(P, a, x, y));
            }
        for (int x = 0; x < 6; x++)
            for (int y = 0; y < 6; y++)
                T.ext[a][x][y] = F(ext_stem_energy(P, a, x == 5 ? -1 : x, y == 5 ? -1 : y));
        T.termAU[a] = F(a > 2 ? P.TermAU : 0);
        for (int b = 1; b <= 7; b++)
            for (int x = 0; x < 5; x++)
                for (int y = 0; y < 5; y++) {
                    T.int11[a][b][x][y] = F(P.int11[a][b][x][y]);
                    for (int z = 0; z < 5; z++) {
                        T.int21[a][b][x][y][z] = F(P.int21[a][b][x][y][z]);
                        for (int w = 0; w < 5; w++)
                            T.int22[a][b][x][y][z][w] = F(P.int22[a][b][x][y][z][w]);
                    }
                }
    }
}

struct Motif {
    std::string seq, fold;
    double energy_kcal = 0.0;
    int mode = ADX_MOTIF_AUTO;   // the per-fold facade too: RNAfold's -9.22 holo MFE
    bool present = false;
};

// Validate the ligand motif and compute its intrinsic energy (kcal/mol).
inline adx_status prepare_motif(const EnergyParams &P, const Motif &m, double &eint, std::vector<int> &pt,
                                SetupError &err) {
    const int L = static_cast<int>(m.seq.size());
    if (L < 5 || L > MAX_MOTIF || static_cast<int>(m.fold.size()) != L)
        return setup_fail(err, ADX_EINVAL, "motif: sequence and fold must have equal length in [5, %d]", MAX_MOTIF);
    if (m.fold.find('&') != std::string::npos)
        return setup_fail(err, ADX_EUNSUPPORTED, "motif: split (&) interior-loop motifs are not supported");
    pt.assign(L, -1);
    std::vector<int> stk;
    for (int k = 0; k < L; k++) {
        if (m.fold[k] == '(') stk.push_back(k);
        else if (m.fold[k] == ')') {
            if (stk.empty()) return setup_fail(err, ADX_EINVAL, "motif: unbalanced fold '%s'", m.fold.c_str());
            pt[stk.back()] = k;
            pt[k] = stk.back();
            stk.pop_back();
        } else if (m.fold[k] != '.') {
            return setup_fail(err, ADX_EINVAL, "motif: bad character in fold '%s'", m.fold.c_str());
        }
    }
    if (!stk.empty()) return setup_fail(err, ADX_EINVAL, "motif: unbalanced fold '%s'", m.fold.c_str());
    if (pt[0] != L - 1)
        return setup_fail(err, ADX_EUNSUPPORTED, "motif: the outermost pair must span the whole motif");
    // every pair canonical, every hairpin >= TURN, every interior loop <= MAXLOOP
    for (int k = 0; k < L; k++) {
        if (pt[k] > k) {
            if (!pair_type(base_code(m.seq[k]), base_code(m.seq[pt[k]])))
                return setup_fail(err, ADX_EINVAL, "motif: non-canonical pair (%d,%d)", k, pt[k]);
            if (pt[k] - k - 1 < TURN) return setup_fail(err, ADX_EINVAL, "motif: hairpin shorter than 3");
            int nb = 0, p = -1, q = -1;
            for (int t = k + 1; t < pt[k]; t++)
                if (pt[t] > t) {
                    if (++nb == 1) { p = t; q = pt[t]; }
                    t = pt[t];
                }
            if (nb == 1 && (p - k - 1) + (pt[k] - q - 1) > MAXLOOP)
                return setup_fail(err, ADX_EUNSUPPORTED, "motif: interior loop larger than MAXLOOP");
        }
    }
    eint = eval_structure(P, m.seq, m.fold);
    if (std::isnan(eint)) return setup_fail(err, ADX_EINVAL, "motif: cannot evaluate fold");
    return ADX_OK;
}

template <class FT>
inline void build_scaled(const EnergyParams &P, double sigma, const Motif &m, double eint,
                         const std::vector<int> &mpt, DevScaledT<FT> &X, bool mfe) {
    std::memset(&X, 0, sizeof X);
    const Fac<FT> F{mfe, sigma};
    auto sp = [&](int k) { return std::pow(sigma, k); };
    FT *ct = X.ctab;
    // code = rtype*25 + S[q+1]*5 + S[p-1] of an inner pair; mismatchI[type2][sq1][sp1]
    for (int code = 0; code < 200; code++) {
        const int t2 = code / 25, x = (code / 5) % 5, y = code % 5;
        if (mfe) {   // energies: the inverse factor is the negated mismatch
            const int mm = t2 ? P.mmI[t2][x][y] : 0;
            ct[CT_INVMM + code] = t2 ? static_cast<FT>(-mm) : FT(MFE_BIG);
            ct[CT_BUL + code] = t2 ? static_cast<FT>(-mm + (t2 > 2 ? P.TermAU : 0)) : FT(MFE_BIG);
            ct[CT_ONEN + code] = t2 ? static_cast<FT>(-mm + P.mm1nI[t2][x][y]) : FT(MFE_BIG);
            ct[CT_M23O + code] = t2 ? static_cast<FT>(P.mm23I[t2][x][y]) : FT(MFE_BIG);
            continue;
        }
        const double mm = t2 ? boltz_d(P.mmI[t2][x][y]) : 0.0;
        const double inv = (mm > 0.0) ? 1.0 / mm : 0.0;
        ct[CT_INVMM + code] = static_cast<FT>(inv);
        ct[CT_BUL + code] = static_cast<FT>(inv * (t2 ? boltz_d(t2 > 2 ? P.TermAU : 0) : 0.0));
        ct[CT_ONEN + code] = static_cast<FT>(inv * (t2 ? boltz_d(P.mm1nI[t2][x][y]) : 0.0));
        ct[CT_M23O + code] = static_cast<FT>(t2 ? boltz_d(P.mm23I[t2][x][y]) : 0.0);
    }
    for (int a = 0; a < 8; a++)
        for (int b = 0; b < 8; b++) ct[CT_STK + a * 8 + b] = (a && b) ? F(P.stack[a][b]) : F.zero();
    for (int u = 0; u < 32; u++) {
        const int uu = std::min(u, MAXLOOP);
        ct[CT_FB + u] = F(P.bulge[uu], u + 2);
        const int nl = u;
        const double e1n = (nl >= 1 && nl + 1 <= MAXLOOP)
                               ? P.interior[nl + 1] + std::min(P.maxninio, (nl - 1) * P.ninio)
                               : INF_E;
        ct[CT_F1N + u] = F(e1n, nl + 3);
    }
    ct[CT_FSM + 0] = F(0, 2);
    ct[CT_FSM + 1] = F(P.bulge[1], 3);
    ct[CT_FSM + 2] = F(0, 4);
    ct[CT_FSM + 3] = F(0, 5);
    ct[CT_FSM + 4] = F(0, 6);
    ct[CT_FSM + 5] = F(P.interior[5] + P.ninio, 7);
    ct[CT_FSM + 6] = F(P.TermAU);
    ct[CT_ONE] = F.one();
    for (int u = 6; u <= MAXLOOP; u++)
        for (int n1 = 2; n1 < 2 + FG_ROW; n1++) {
            const int n2 = u - n1;
            X.fgen[(u - 6) * FG_ROW + n1 - 2] =
                n2 >= 2 ? F(P.interior[u] + std::min(P.maxninio, std::abs(n1 - n2) * P.ninio), u + 2) : F.zero();
        }
    for (int k = 0; k < 32; k++) {
        X.il[k] = (mfe && k <= MAXLOOP) ? static_cast<FT>(P.interior[k]) : FT(0);
        X.nin[k] = mfe ? static_cast<FT>(std::min(P.maxninio, k * P.ninio)) : FT(0);
    }
    // term lists ordered by u (dev_types.hpp NS_MAX)
    int ns = 0, ng = 0;
    auto addS = [&](int kind, int n1, int n2, FT f) {
        X.s_kind[ns] = static_cast<uint8_t>(kind);
        X.s_n1[ns] = static_cast<uint8_t>(n1);
        X.s_n2[ns] = static_cast<uint8_t>(n2);
        X.s_f[ns] = f;
        ns++;
    };
    for (int u = 0; u <= MAXLOOP; u++) {
        if (u == 0) addS(TK_STK, 0, 0, ct[CT_FSM + 0]);
        if (u == 1) { addS(TK_B1, 0, 1, ct[CT_FSM + 1]); addS(TK_B1, 1, 0, ct[CT_FSM + 1]); }
        if (u == 2) addS(TK_I11, 1, 1, ct[CT_FSM + 2]);
        if (u == 3) { addS(TK_I12, 1, 2, ct[CT_FSM + 3]); addS(TK_I21, 2, 1, ct[CT_FSM + 3]); }
        if (u == 4) addS(TK_I22, 2, 2, ct[CT_FSM + 4]);
        if (u == 5) { addS(TK_M23, 2, 3, ct[CT_FSM + 5]); addS(TK_M23, 3, 2, ct[CT_FSM + 5]); }
        if (u >= 2) { addS(TK_BUL, 0, u, ct[CT_FB + u]); addS(TK_BUL, u, 0, ct[CT_FB + u]); }
        if (u >= 4) { addS(TK_1N, 1, u - 1, ct[CT_F1N + u - 1]); addS(TK_1N, u - 1, 1, ct[CT_F1N + u - 1]); }
        for (int n1 = 2; u >= 6 && n1 <= u - 2; n1++) {
            X.g_n1[ng] = static_cast<uint8_t>(n1);
            X.g_u[ng] = static_cast<uint8_t>(u);
            X.g_f[ng] = X.fgen[(u - 6) * FG_ROW + n1 - 2];
            ng++;
        }
        X.s_cnt[u] = ns;
        X.g_cnt[u] = ng;
    }
    X.s_cnt[31] = ns;
    X.g_cnt[31] = ng;
    for (int k = 0; k < NMAX + 4; k++) X.sig[k] = F(0, k);
    for (int u = 0; u <= NMAX; u++) {
        if (mfe) {   // the MFE truncates the long-loop extrapolation to dcal (oracle E_hairpin_int)
            const int e = (u <= 30) ? P.hairpin[u] : P.hairpin[30] + static_cast<int>(P.lxc * std::log(u / 30.0));
            X.hp[u] = F(e);
        } else {
            const double e = (u <= 30) ? P.hairpin[u] : P.hairpin[30] + P.lxc * std::log(u / 30.0);
            X.hp[u] = F(e, u + 2);
        }
    }
    const double mlb = boltz_d(P.MLbase);
    for (int t = 0; t <= NMAX; t++)
        X.pwml[t] = mfe ? static_cast<FT>(t * P.MLbase) : static_cast<FT>(std::pow(mlb * sigma, t));
    X.mlclosing = F(P.MLclosing, 2);
    X.mlbase_sig = F(P.MLbase, 1);
    int nsp = 0;
    auto add_special = [&](const std::vector<std::pair<std::string, int>> &tab) {
        for (auto &e : tab) {
            if (nsp >= MAX_SPECIAL_HP) break;
            std::vector<uint8_t> codes(e.first.size());
            for (size_t k = 0; k < e.first.size(); k++) codes[k] = static_cast<uint8_t>(base_code(e.first[k]));
            X.sp_key[nsp] = hp_key(codes.data(), 0, static_cast<int>(codes.size()));
            X.sp_val[nsp] = F(e.second, static_cast<int>(codes.size()));
            nsp++;
        }
    };
    add_special(P.triloops);
    add_special(P.tetraloops);
    add_special(P.hexaloops);
    X.n_special = nsp;
    X.log_sigma = mfe ? 0.0 : std::log(sigma);
    X.kT = kT_kcal();
    if (m.present) {
        const int L = static_cast<int>(m.seq.size());
        X.motif_len = L;
        for (int k = 0; k < L; k++) {
            X.motif_code[k] = static_cast<uint8_t>(base_code(m.seq[k]));
            X.motif_pt[k] = static_cast<int8_t>(mpt[k]);
        }
        const bool replace = m.mode == ADX_MOTIF_REPLACE || (m.mode == ADX_MOTIF_AUTO && mfe);
        const double beff = replace ? m.energy_kcal - eint : m.energy_kcal;
        if (mfe) {   // min-plus image of the extra term: the formed motif's energy, rounded once to dcal
            X.motif_extra = static_cast<FT>(std::lround(100.0 * (eint + beff)));
        } else {
            const double extra = boltz_d(eint * 100.0) * (boltz_d(beff * 100.0) - 1.0) * sp(L);
            X.motif_extra = static_cast<FT>(extra);
        }
    }
}

// struct_eval_kernel's table (dev_types.hpp EvalTab) in the PF (mfe false) or
// MFE convention; the motif as build_scaled reads it (AUTO: ADD in PF, REPLACE in MFE)
inline void build_eval_tab(const EnergyParams &P, const Motif &m, double eint, EvalTab &E, bool mfe) {
    std::memset(&E, 0, sizeof E);
    const int *tab[3] = {P.hairpin, P.bulge, P.interior};
    for (int kind = 0; kind < 3; kind++)
        for (int u = 0; u <= NMAX; u++) {
            if (u <= 30) E.len[kind][u] = tab[kind][u];
            else if (mfe) E.len[kind][u] = tab[kind][30] + static_cast<int>(P.lxc * std::log(u / 30.0));
            else E.len[kind][u] = tab[kind][30] + P.lxc * std::log(u / 30.0);
        }
    for (int k = 0; k <= NMAX; k++) E.nin[k] = std::min(P.maxninio, k * P.ninio);
    int nsp = 0;
    for (const auto *t : {&P.triloops, &P.tetraloops, &P.hexaloops})
        for (const auto &e : *t)
            if (nsp < MAX_SPECIAL_HP) E.sp_e[nsp++] = e.second;
    E.mlclosing = P.MLclosing;
    E.mlbase = P.MLbase;
    E.mfe = mfe ? 1 : 0;
    E.kT = kT_kcal();
    if (m.present) {
        const bool replace = m.mode == ADX_MOTIF_REPLACE || (m.mode == ADX_MOTIF_AUTO && mfe);
        E.m_eint = eint;
        E.m_beff = replace ? m.energy_kcal - eint : m.energy_kcal;
        E.m_mfe_dcal = static_cast<int>(std::lround(100.0 * (eint + E.m_beff)));
    }
}

// Dot-bracket hard constraint (DB_DEFAULT | ENFORCE_BP, scoring.cc:61-62) ->
// five byte arrays of length N+2: up, dn, ptn, enc, flg (see fold_common.hpp allowed()).
inline adx_status build_constraint(const std::string &cst, int N, std::vector<uint8_t> &out, SetupError &err) {
    const int np = N + 2;
    out.assign(5 * np, 0);
    std::vector<int> partner(np, 0), enc(np, 0), unp(np, 1), flg(np, 0), stk;
    for (int i = 1; i <= N; i++) {
        const char c = cst.empty() ? '.' : cst[i - 1];
        enc[i] = stk.empty() ? 0 : stk.back();
        if (c == '(') stk.push_back(i);
        else if (c == ')') {
            if (stk.empty()) return setup_fail(err, ADX_ECONSTRAINT, "unbalanced ')' in constraint '%s'", cst.c_str());
            int a = stk.back();
            stk.pop_back();
            partner[a] = i;
            partner[i] = a;
            enc[i] = stk.empty() ? 0 : stk.back();
        }
    }
    if (!stk.empty()) return setup_fail(err, ADX_ECONSTRAINT, "unbalanced '(' in constraint '%s'", cst.c_str());
    for (int i = 1; i <= N; i++) {
        const char c = cst.empty() ? '.' : cst[i - 1];
        if (c == 'x') flg[i] |= 1;
        if (c == '<') flg[i] |= 2;
        if (c == '>') flg[i] |= 4;
        if (c == '|') flg[i] |= 8;
        if (c == '|' || c == '<' || c == '>' || partner[i]) unp[i] = 0;
    }
    std::vector<int> up(np + 1, 0), dn(np, 0);
    for (int i = N; i >= 1; i--) up[i] = unp[i] ? up[i + 1] + 1 : 0;
    for (int i = 1; i <= N; i++) dn[i] = unp[i] ? dn[i - 1] + 1 : 0;
    for (int k = 0; k < np; k++) {
        out[k] = static_cast<uint8_t>(std::min(up[k], 255));
        out[np + k] = static_cast<uint8_t>(std::min(dn[k], 255));
        out[2 * np + k] = static_cast<uint8_t>(partner[k]);
        out[3 * np + k] = static_cast<uint8_t>(enc[k]);
        out[4 * np + k] = static_cast<uint8_t>(flg[k]);
    }
    return ADX_OK;
}

inline std::vector<uint8_t> encode(const std::string &s) {
    std::vector<uint8_t> v(s.size());
    for (size_t k = 0; k < s.size(); k++) v[k] = static_cast<uint8_t>(base_code(s[k]));
    return v;
}

inline const char *move_error_text(int code) {
    switch (code) {
    case 1: return "mismatched base-pair in macrostate";
    case 2: return "position can be mutated, but it's base-paired to a position which can't be";
    case 3: return "no way to satisfy all base pairing constraints.";
    default: return "unknown move error";
    }
}

// mutate_recursively (sampling.cc:195-282) on the template, recording the
// closure of `pos` with its base parity and the first error the reference
// would throw.  The result does not depend on the base chosen.
inline int closure(const std::string &seq, const std::vector<std::string> &ms, int pos,
                   std::vector<std::pair<int, int>> &out) {
    const int n = static_cast<int>(seq.size());
    std::vector<int> par(n, -1);
    // recursive DFS in the reference's order
    std::function<int(int, int)> rec = [&](int p, int parity) -> int {
        par[p] = parity;
        out.push_back({p, parity});
        for (const auto &mac : ms) {
            char open, close;
            int stepv;
            if (mac[p] == '(') { open = '('; close = ')'; stepv = 1; }
            else if (mac[p] == ')') { open = ')'; close = '('; stepv = -1; }
            else continue;
            int level = 1, partner = p;
            while (level != 0) {
                partner += stepv;
                if (partner < 0 || partner >= n) return 1;
                level += (mac[partner] == open);
                level -= (mac[partner] == close);
            }
            if (!std::isupper(static_cast<unsigned char>(seq[partner]))) return 2;
            if (par[partner] < 0) {
                int rc = rec(partner, parity ^ 1);
                if (rc) return rc;
            } else if (par[partner] != (parity ^ 1)) {
                return 3;
            }
        }
        return 0;
    };
    return rec(pos, 0);
}

// MFE: the energy tables as packed int16 pairs (value duplicated in both
// halves; >= MFE_BIG/2 -> 0x7FFF).  Returns false when a value does not fit.
inline bool pack16(float *a, size_t n) {
    for (size_t k = 0; k < n; k++) {
        const double e = a[k];
        uint32_t h;
        if (e >= 0.5 * MFE_BIG) h = 0x7FFFu;
        else if (e <= -16384.0 || e >= 16384.0 || e != std::floor(e)) return false;
        else h = static_cast<uint16_t>(static_cast<int16_t>(e));
        const uint32_t w = h | (h << 16);
        std::memcpy(&a[k], &w, 4);
    }
    return true;
}

// T16 / X16: copies of the MFE tables, packed in place, with X16's ku16 records.
// False when a value does not fit (FP32 MinPlus only).
inline bool pack_mfe16(DevTables &T16, DevScaled &X16) {
    bool ok = pack16(reinterpret_cast<float *>(&T16), sizeof(DevTables) / sizeof(float));
    ok = ok && pack16(X16.ctab, CT_SIZE) && pack16(X16.fgen, FG_SIZE) && pack16(X16.il, 32) && pack16(X16.nin, 32) && pack16(X16.s_f, NS_MAX) &&
         pack16(X16.g_f, NG_MAX) && pack16(X16.sig, NMAX + 4) && pack16(X16.hp, NMAX + 1) &&
         pack16(X16.pwml, NMAX + 1) && pack16(&X16.mlclosing, 1) && pack16(&X16.mlbase_sig, 1) &&
         pack16(X16.sp_val, MAX_SPECIAL_HP) && pack16(&X16.motif_extra, 1);
    if (!ok) return false;
    // mfe_cells.hip interior-loop records (both halves non-negative: a plain 32-bit add)
    uint32_t il[32], nin[32], ct[CT_SIZE];
    std::memcpy(il, X16.il, sizeof il);
    std::memcpy(nin, X16.nin, sizeof nin);
    std::memcpy(ct, X16.ctab, sizeof ct);
    for (int u = 0; u < 32; u++)
        for (int f = 0; f < 8; f++)
            X16.ku16[u][f] = f < 6 ? ((u >= 6 && u <= 30) ? il[u] + nin[f] : 0u)
                            : f == 6 ? ct[CT_FB + u] : (u >= 1 ? ct[CT_F1N + u - 1] : 0x7FFF7FFFu);
    return true;
}

// the energy models the lanes = cells MFE kernel covers (mfe_cells.hip):
// MLbase >= 0, Ninio saturated from |n1-n2| = 5 on
inline bool mfe_cells_model_ok(const EnergyParams &P) {
    bool ok = P.MLbase >= 0;
    for (int k = 5; k <= MAXLOOP; k++)
        if (std::min(P.maxninio, k * P.ninio) != std::min(P.maxninio, 5 * P.ninio)) ok = false;
    return ok;
}

// apo / holo variants of one (context, macrostate) share every cell: pair them
// (fold_rows.hip pf_group; a lone variant is paired with itself)
inline std::vector<int> pair_groups2(const std::vector<DevVariant> &variants, const std::vector<int> &vmac) {
    std::vector<int> groups2;
    std::vector<char> used(variants.size(), 0);
    for (size_t v = 0; v < variants.size(); v++) {
        if (used[v]) continue;
        used[v] = 1;
        size_t mate = v;
        for (size_t w = v + 1; w < variants.size(); w++) {
            if (!used[w] && variants[w].ctx == variants[v].ctx && vmac[w] == vmac[v] &&
                variants[w].N == variants[v].N && variants[w].motif != variants[v].motif) {
                mate = w;
                used[w] = 1;
                break;
            }
        }
        groups2.push_back(static_cast<int>(v));
        groups2.push_back(static_cast<int>(mate));
    }
    return groups2;
}

// every outside variant's position in the groups2 slot layout (the outside
// kernels read the proposal's inside tables there): an invariant, not a search
inline adx_status outside_slots(const std::vector<int> &groups2, const std::vector<int> &bvars,
                                std::vector<int> &bslot, SetupError &err) {
    bslot.assign(bvars.size(), -1);
    for (size_t b = 0; b < bvars.size(); b++)
        for (size_t g = 0; g < groups2.size() && bslot[b] < 0; g++)
            if (groups2[g] == bvars[b]) bslot[b] = static_cast<int>(g);
    for (size_t b = 0; b < bslot.size(); b++)
        if (bslot[b] < 0)
            return setup_fail(err, ADX_EINVAL, "internal: outside variant %d has no fold group", bvars[b]);
    return ADX_OK;
}

}  // namespace adx
