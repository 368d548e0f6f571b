// gfx950 minimum-free-energy fold for the Monte Carlo score (BASELINE
// configs[1]) with TWO anti-diagonals per barrier.  The recursion, the tables
// and the lanes = cells mapping are those of mfe_cells.hip (Zuker MFE of the
// ViennaRNA-2.x default model, dangles = 2, hard constraints, ligand motif;
// oracle/fold.c orc_mfe_energy; apo | holo packed as 16-bit halves); what
// changes is the step's dependency structure, so that one barrier serves two
// diagonals and a B lane-set holds the pairable cells of both:
//
// Step d (d = 6, 8, ...; one barrier at its end):
//   F  finalize e0 = d-2 and e1 = d-1, lanes = rows i, two cells per lane:
//      c = min(B's partials (loop sizes u >= 2), the stack and bulge-1 shapes
//      (inner spans e-2, e-3: final a step earlier), hairpin / motif,
//      multiloop closing mla(i+1, j-1) + closing), qbm = c + mismatchI,
//      qm1 = min(c + stem, qm1(i, j-1) + MLbase) (cell e1 takes cell e0's qm1
//      from the same lane), the unpaired part of qm
//      U(i, j) = min(qm1(i, j), U(i+1, j) + MLbase) (cell e1 takes U of row
//      i+1 from the next lane), qm = min(split, U).  A refold runs only the
//      rows it rewrites and one ghost row above them, whose restored qm stands
//      in for its U (see F below); a window of at most 32 rows runs one cell
//      per lane, the two cells of a row on the two halves of the wave
//   B  interior-loop partials of diagonals d and d+1, loop sizes u >= 2
//      (inner spans <= d-3: final a step earlier), one lane-set over the
//      pairable cells of both; every block wave folds its partial into the
//      cell's slot with an LDS atomic min (apo and holo halves apart)
//   M  split parts of qm for spans d, d+1 (they read spans <= d-4)
//   Q  q5[d-3] and q5[d-2] in one pass over k
//   L  the pairable cells of diagonals d+2, d+3 and their B records
// Everything a phase reads was written one step earlier or before the loop,
// so the 97 diagonals of a 100-nt fold take 49 barriers instead of 97, and the
// step's fixed costs (records, counts, the B cell setup, the roles' round
// trips) are paid once per two diagonals.
//
// Every stored value goes through pfin() as in mfe_cells.hip.
//
// The file in reading order: the carve (CP, PLay), pair_setup (sequence, tables,
// refold restore, per-cell pass; one copy for all waves), one function per role
// (build_list / load_list, finalize on FRun, block_partials, split_rows,
// q5_columns), mfe_pair_fold (the step loop, one instance per wave), the kernel
// and its launcher.  mfe_common.hpp holds what mfe_cells.hip spells alike.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "dev_types.hpp"
#include "fold_common.hpp"
#include "launch.hpp"
#include "mfe_common.hpp"

namespace adx {

#define PSTAMP(k) ADX_STAMP_AT(k)   // fold_common.hpp
#ifdef ADX_STAMP
// the roles that stamp inside take the sweep's counters
#define PSTAMP_PARAMS , unsigned long long *st_acc, unsigned long long &st_last
#define PSTAMP_ARGS , st_acc, st_last
__device__ unsigned long long g_stamps_p[16][16];
// the same sums as they stand after the early steps (span e0 = d - 2 has more than
// 64 rows, so a fold from scratch finalizes in two lane-sets): the share of those
// steps, which tells the wave that sets them
__device__ unsigned long long g_stamps_pe[16][16];
#else
#define PSTAMP_PARAMS
#define PSTAMP_ARGS
#endif

namespace {

// waves per walker: 0..6 interior-loop blocks, 7 the finalize; the split parts
// of qm (one span per wave), the lists and q5 ride on block waves, whose loop
// sizes the generator partitions around them (tools/gen_mfe_blocks.py
// PAIR_ROLES4; two workgroups per CU)
// eight waves, NWV in mfe_common.hpp (ten waves with nine blocks measured
// -37 %: a 10-wave workgroup's waves land 3, 3, 2, 2 on the SIMDs, so a second
// one does not fit at 96 VGPRs)
constexpr int PAIR_NBLK = 7;   // (a block on the finalize wave too, 8, measured -5.7 %: the finalize
                               // wave then sets the step)
constexpr int PRIO_ROLE = 2;   // s_setprio of the one-wave roles over the block waves
// the waves of the one-wave roles
constexpr int F_WAVE = 7;
constexpr int L_WAVE = 1;            // the lists two steps ahead (diagonals d+4, d+5) and their B records
                                     // (round 5: wave 1 +0.8 % over wave 4, A/B r05zn/r05zo)
constexpr int Q_WAVE = 3;            // q5 of two columns (on the finalize wave: -2.1 %, A/B r06n)
constexpr int FW[2] = {F_WAVE, 6};   // finalize lane-sets 0, 1 (the first 64 rows, the rest): lane-set 1
                                     // (a fold from scratch at spans < 38; a refold whose row window
                                     // is longer, i.e. both partners of an enforced pair changed)
                                     // rides on block wave 6
constexpr int MW[2] = {0, 2};        // the split parts of spans d, d+1

#include "mfe_pair_blocks.inc"
static_assert(MFE_NBLK == PAIR_NBLK, "one block per block wave");

constexpr int PINF = 32767;   // an impossible half, sign-extended (the partial slots)

// bit 8 * log2(lanes per cell) + b: block b reads loop size u in that mode
constexpr unsigned size_bits(int u) {
    unsigned m = 0;
    for (int s = 0; s < 3; s++)
        if (MFE_SIZE_BLOCK[s][u] >= 0) m |= 1u << (8 * s + MFE_SIZE_BLOCK[s][u]);
    return m;
}

// ---------------------------------------------------------------- LDS carve
struct CP {
    u32 *qbm, *qm, *qm1;   // cell tables (fold_common.hpp indexing); qbm has an
                           // impossible "span 3" diagonal right before it
    int *part;             // [4][2][np]: B's partial minima of a diagonal (span & 3) by row,
                           //   apo / holo halves sign-extended (ds_min_i32)
    u32 *mla;              // [6][np]: split part of qm by span % 6, by row
    u32 *colmin;           // [4][np]: U(j - span, j) by span & 3, by column j
    u32 *q5;               // [np]
    u32 *ct;               // CT_SIZE (DevScaled::ctab, packed)
    u32 *dt;               // DT_* block (packed)
    uint8_t *cc;           // inner-pair code per cell (diagonal-major), pad before it
    uint8_t *S, *up, *dn, *ptn, *enc, *flg, *mat, *raw;
    u32 *pos;              // [np]: S | flg << 3 | up << 8 | ptn << 16 | enc << 24 (the per-cell pass)
    uint8_t *cl;           // [3][2 np]: rows of the pairable cells of a step's two diagonals, by step % 3
    int *cnt;              // [3]: cells of the step's first diagonal | of both << 16
    int *flag;             // [3]: block_or words (constrained, 16-bit range left), the item's queue index
    u32 *rec;              // [3][2][64]: the B cells' setup (rank < 64 over both diagonals) by step % 3:
                           //   i | oc << 8 | A << 16 | B << 24 and mismatchI(oc) | mismatch1n(oc) +
                           //   mismatchI(oc) << 16 (MFE table entries are equal in both halves)
    u32 *e4;               // [MFE_E4_SLOTS][4]: per-slice generic energies of the 4-lane blocks
    int np;
};

template <int NM>
struct PLay {
    static constexpr int NP = NM + 2;
    static constexpr size_t C = size_t(NM - 4) * (NM - 3) / 2;
    static constexpr size_t PADQ = al16(size_t(NM - 3) * 4);   // the span-3 diagonal of qbm (impossible)
    static constexpr size_t QBM = PADQ;
    static constexpr size_t QM = QBM + al16(C * 4);
    static constexpr size_t QM1 = QM + al16(C * 4);
    static constexpr size_t PART = QM1 + al16(C * 4);          // PART, MLA, CMN: the setup's scratch too
    static constexpr size_t MLA = PART + al16(4 * 2 * NP * 4);
    static constexpr size_t CMN = MLA + al16(6 * NP * 4);
    static constexpr size_t Q5 = CMN + al16(4 * NP * 4);
    static constexpr size_t CT = Q5 + al16(NP * 4);
    static constexpr size_t DT = CT + al16(CT_SIZE * 4);
    static constexpr size_t CC = DT + al16(size_t(DT_HP) * 4) + al16(NM - 3);   // span-3 codes before it
    static constexpr size_t BY = CC + al16(C);
    static constexpr size_t CLS = BY + al16(8 * NP);
    static constexpr size_t CNT = CLS + al16(6 * NP);
    static constexpr size_t FLAG = CNT + 16;
    static constexpr size_t REC = FLAG + 16;
    static constexpr size_t E4 = REC + 3 * 2 * 64 * 4;
    static constexpr size_t POS = E4 + size_t(MFE_E4_MAX) * 16;
    static constexpr size_t BYTES = POS + al16(size_t(NP) * 4);
    __device__ static CP carve() {   // LDS addresses as literals (no static LDS: the dynamic block starts at 0)
        CP l;
        l.qbm = lds_at<u32>(QBM);
        l.qm = lds_at<u32>(QM);
        l.qm1 = lds_at<u32>(QM1);
        l.part = lds_at<int>(PART);
        l.mla = lds_at<u32>(MLA);
        l.colmin = lds_at<u32>(CMN);
        l.q5 = lds_at<u32>(Q5);
        l.ct = lds_at<u32>(CT);
        l.dt = lds_at<u32>(DT);
        l.cc = lds_at<uint8_t>(CC);
        carve_bytes(l, lds_at<uint8_t>(BY), NP);
        l.cl = lds_at<uint8_t>(CLS);
        l.cnt = lds_at<int>(CNT);
        l.flag = lds_at<int>(FLAG);
        l.rec = lds_at<u32>(REC);
        l.e4 = lds_at<u32>(E4);
        l.pos = lds_at<u32>(POS);
        l.np = NP;
        return l;
    }
};
static_assert(MFE_E4_SLOTS <= MFE_E4_MAX, "CP::e4 holds the generated slots");

// variant v's words (global loads: fold_common.hpp gld)
__device__ __forceinline__ DevVariant variant_at(const KArgs &ka, int v) {
    const DevVariant *p = ka.variants + v;
    return DevVariant{gld(&p->N), gld(&p->before_len), gld(&p->ctx), gld(&p->cons_off), gld(&p->motif), 0};
}

__device__ __forceinline__ int sext_lo(u32 x) { return int(short(x & 0xFFFFu)); }
__device__ __forceinline__ int sext_hi(u32 x) { return int(x) >> 16; }
__device__ __forceinline__ u32 pack2(int lo, int hi) { return (u32(lo) & 0xFFFFu) | (u32(hi) << 16); }

// The per-cell setup of quarter-sets 4 I0 .. 4 I0 + 15 (as in mfe_cells.hip):
// inner-pair code, hairpin (+ motif) or the non-pairable mark, multiloop stem
// of the pairable cells, for the changed band
// (a fold from scratch: every cell; a refold restored the others).  Round 6:
// the band's rows in quarter-sets of 16 (diagonal d, rows clo(d) + 16c ..), four
// quarter-sets per 64-lane item and four items per batch, each batch in two LDS
// round trips; items by diagonal left most lanes idle (a refold's band holds
// d + 3 rows of diagonal d) and took three times the batches
// qtab, tot: the quarter-set table; hpf: hairpin length factors; spk, spv: special hairpins
__device__ __forceinline__ void cell_pass(const CP &L, const Band &bd, int lane, int I0, const u32 *qtab, int tot,
                                          const u32 *hpf, const uint32_t *spk, const u32 *spv, int mL, u32 mextra) {
    const int N = bd.N;
    constexpr int NI = 4;   // items I0 .. I0 + 3 (quarter-sets 4 I .. 4 I + 3, lanes 16 g ..)
    int ii[NI], jj[NI], dv[NI];
    bool ok[NI];
    u32 wim[NI], wi[NI], wi1[NI], wjm[NI], wj[NI], wjp[NI];
    uint32_t mt[NI];
#pragma unroll
    for (int q = 0; q < NI; q++) {
        const int k = 4 * (I0 + q) + (lane >> 4);   // the lane's quarter-set
        const u32 e = qtab[k < tot ? k : 0];
        const int d = k < tot ? int(e & 255) : 4;
        const int r = int(e >> 8) + (lane & 15) - 1;
        const bool v = k < tot && r < bd.chi(d);
        dv[q] = d;
        ok[q] = v;
        const int i = ok[q] ? r + 1 : 1, j = ok[q] ? i + d : 5;
        ii[q] = i;
        jj[q] = j;
        wim[q] = L.pos[i - 1];
        wi[q] = L.pos[i];
        wi1[q] = L.pos[i + 1];
        wjm[q] = L.pos[j - 1];
        wj[q] = L.pos[j];
        wjp[q] = L.pos[j + 1];
        mt[q] = L.mat[i];
    }
    int ty[NI], ix1[NI];
    bool pr[NI], inb[NI];
    u32 f1[NI], f2[NI], hv[NI];
#pragma unroll
    for (int q = 0; q < NI; q++) {
        const int i = ii[q], j = jj[q], d = dv[q];
        hv[q] = hpf[d - 1];
        const int si = wi[q] & 7, sj = wj[q] & 7;
        ty[q] = ptype(si, sj);
        inb[q] = ok[q];
        const int fi = (wi[q] >> 3) & 7, fj = (wj[q] >> 3) & 7;
        const int pi = (wi[q] >> 16) & 255, pj = (wj[q] >> 16) & 255;
        bool al = !((fi | fj) & 1) && !((fi & 2) || (fj & 4));
        al = al && (pi ? pi == j : (pj ? pj == i : (wi[q] >> 24) == (wj[q] >> 24)));
        pr[q] = inb[q] && ty[q] != 0 && al;
        const int sim = wim[q] & 7, sjp = wjp[q] & 7, si1 = wi1[q] & 7, sjm = wjm[q] & 7;
        ix1[q] = hairpin_dt_index(d - 1, ty[q], si1, sjm);
        f1[q] = L.dt[ix1[q]];
        f2[q] = L.dt[DT_MLS + ty[q] * 25 + sim * 5 + sjp];
    }
#pragma unroll
    for (int q = 0; q < NI; q++) {
        const int i = ii[q], j = jj[q], d = dv[q], u = d - 1;
        if (!ok[q]) continue;
        L.cc[off(d, N) + i - 1] = static_cast<uint8_t>(rtype(ty[q]) * 25 + (wjp[q] & 7) * 5 + (wim[q] & 7));
        u32 h = INF16;
        if (((wi1[q] >> 8) & 255) >= uint32_t(u)) {
            h = padd(hv[q], f1[q]);
            if (u == 3 || u == 4 || u == 6) {   // special hairpins (three diagonals)
                const int sh = special_hp(spk, hp_key(L.S, i, u + 2));
                if (sh >= 0) h = spv[sh];
            }
        }
        if (d == mL - 1 && mL > 0 && mt[q]) h = pmin(h, mextra);
        if (inb[q]) {
            L.qbm[off(d, N) + i - 1] = pr[q] ? h : MARK16;
            L.qm1[colb(j) + i - 1] = pr[q] ? f2[q] : INF16;
        }
    }
}

// What is the same for every fold of a launch, stored once per workgroup before
// its first item (no fold writes these regions): the energy tables ct, dt and e4
// (the generic interior energies of the 4-lane blocks) and the impossible span-3
// diagonal in front of qbm with its codes in front of cc.  Every load is in flight
// before the first store; the caller's next barrier orders the stores.
template <int NT, int NM>
__device__ __forceinline__ void pair_constants(const DevScaled *__restrict__ XS, const DevTables *__restrict__ TT,
                                               const CP &L) {
    static_assert(NT >= 288 && NT >= MFE_E4_SLOTS * 4, "one table element per thread");
    const int tid = threadIdx.x;
    const u32 *gct = reinterpret_cast<const u32 *>(XS->ctab);
    constexpr int NCT = (CT_SIZE + NT - 1) / NT;
    u32 v_ct[NCT];
#pragma unroll
    for (int t = 0; t < NCT; t++) v_ct[t] = gld(gct + uint32_t(min(tid + t * NT, CT_SIZE - 1)));
    const DevTables &T0 = *TT;
    const u32 v_mh = __float_as_uint(gld(&T0.mmH[0][0][0] + uint32_t(min(tid, 199))));
    const u32 v_mi = __float_as_uint(gld(&T0.mmI[0][0][0] + uint32_t(min(tid, 199))));
    const u32 v_ms = __float_as_uint(gld(&T0.mlstem[0][0][0] + uint32_t(min(tid, 199))));
    const u32 v_ex = __float_as_uint(gld(&T0.ext[0][0][0] + uint32_t(min(tid, 287))));
    const u32 v_tau = __float_as_uint(gld(T0.termAU + uint32_t(tid & 7)));
    const int ke = min(tid, MFE_E4_SLOTS * 4 - 1);
    const int e4a = MFE_E4_A[ke >> 2][ke & 3], e4u = MFE_E4_U[ke >> 2];
    const u32 v_e4 = gld(&XS->ku16[e4u][max(e4a, 0)]);
#pragma unroll
    for (int t = 0; t < NCT; t++)
        if (tid + t * NT < CT_SIZE) L.ct[tid + t * NT] = v_ct[t];
    if (tid < 200) {
        L.dt[DT_MMH + tid] = v_mh;
        L.dt[DT_MMI + tid] = v_mi;
        L.dt[DT_MLS + tid] = v_ms;
    }
    if (tid < 288) L.dt[DT_EXT + tid] = v_ex;
    if (tid < 8) L.dt[DT_TAU + tid] = v_tau;
    if (tid < MFE_E4_SLOTS * 4) L.e4[tid] = e4a < 0 ? INF16 : v_e4;
    for (int k = tid; k < NM - 3; k += NT) {   // (B's d-lanes reach the span-3 diagonal)
        (L.qbm - (NM - 3))[k] = INF16;
        (L.cc - (NM - 3))[k] = 0;
    }
}

// The fold's setup (sequence, tables, refold restore, per-cell pass) and its
// write-back run in the kernel body, one copy of the code for all eight waves
// (round 6: as part of the per-wave instances each wave fetched its own copy,
// ~1.1k instruction-cache misses per fold group, profiles/r06u_icache_pmc.txt).
// Returns the constrained flag; sst (stamp builds) gets the phase cycles.
template <int NT, int NM>
__device__ __forceinline__ bool pair_setup(const KArgs &ka, const DevScaled *__restrict__ XS,
                                           const DevTables *__restrict__ TT, const int *vs, const uint8_t *raw,
                                           const CP &L, const IncM &inc, const int tid,
                                           unsigned long long *sst) {
    static_assert(NT == NWV * WAVE, "one wave per block slot");
    // (uni(): the kernel's loop makes every load from global memory a vector load)
    DevVariant V = variant_at(ka, vs[0]);
    V.ctx = uni(V.ctx), V.cons_off = uni(V.cons_off);
    const bool mh0 = uni(V.motif) != 0, mh1 = uni(gld(&ka.variants[vs[1]].motif)) != 0;
    const int N = uni(V.N);
    const int lane = tid & (WAVE - 1);
    const int wid = uni(tid / WAVE);
    const int NP = L.np;
#ifdef ADX_STAMP
    const unsigned long long st_setup0 = __builtin_amdgcn_s_memtime();
#endif
    const Band bd = inc.band(N);
    const bool incr = bd.incr;
    const int m_lo = bd.m_lo;

    // ---- setup loads (round 6): every table element and sequence / constraint byte this
    // thread stores, all in flight at once and stored before the restore's loads are
    // issued (the kernel prologue's loop per table waited on each load in turn, and the
    // setup tables' loads waited behind the restore's)
    static_assert(NT >= MAX_SPECIAL_HP && NT >= MAX_MOTIF && NT >= NM + 2, "one setup element per thread");
    const u32 v_hp = __float_as_uint(gld(XS->hp + uint32_t(min(tid, N))));   // hairpin length factors (per-cell pass)
    const int n_sp = uni(gld(&XS->n_special));
    const uint32_t v_spk = gld(XS->sp_key + uint32_t(min(tid, MAX_SPECIAL_HP - 1)));
    const u32 v_spv = __float_as_uint(gld(XS->sp_val + uint32_t(min(tid, MAX_SPECIAL_HP - 1))));
    const uint8_t v_mc = gld(XS->motif_code + uint32_t(min(tid, MAX_MOTIF - 1)));
    const int8_t v_mp = gld(XS->motif_pt + uint32_t(min(tid, MAX_MOTIF - 1)));
    // position k = tid: its base (ViennaRNA's S1 wrap-around at 0 and N + 1) and constraints
    const uint8_t *cons = ka.cons + V.cons_off;
    const int np = N + 2;
    const int kp = min(tid, np - 1);
    uint8_t v_sw, v_up, v_dn, v_pt, v_en, v_fl;
    {
        SeqSrc src{nullptr, raw, nullptr, 0, ka.Nraw};   // seq_src() through gld
        if (V.ctx >= 0) {
            src.bef = ka.ctx_seq + gld(ka.ctx_off + 4 * V.ctx + 0);
            src.blen = gld(ka.ctx_off + 4 * V.ctx + 1);
            src.aft = ka.ctx_seq + gld(ka.ctx_off + 4 * V.ctx + 2);
        }
        v_sw = gld(src.at(wrap_pos(kp, N) - 1));
        v_up = gld(cons + uint32_t(kp));
        v_dn = gld(cons + uint32_t(np + kp));
        v_pt = gld(cons + uint32_t(2 * np + kp));
        v_en = gld(cons + uint32_t(3 * np + kp));
        v_fl = gld(cons + uint32_t(4 * np + kp));
    }
    // ---- the stores: sequence, constraint arrays (mfe_cells.hip), tables
    if (tid < np) {
        L.S[tid] = v_sw;
        L.up[tid] = v_up;
        L.dn[tid] = v_dn;
        L.ptn[tid] = v_pt;
        L.enc[tid] = v_en;
        L.flg[tid] = v_fl;
        L.mat[tid] = 0;
        L.pos[tid] = u32(v_sw) | (u32(v_fl & 7) << 3) | (u32(v_up) << 8) | (u32(v_pt) << 16) | (u32(v_en) << 24);
    }
    const bool cst = tid >= 1 && tid <= N && (v_fl || v_pt);
    u32 *hpf = L.colmin;   // the U slots' space until the sweep (initialised after the per-cell pass)
    static_assert(4 * (NM + 2) >= NM + 1, "hairpin factors fit the U slots");
    if (tid <= N) hpf[tid] = v_hp;
    // setup scratch in the partial / split / U slots (first written after the per-cell pass)
    uint32_t *spk = reinterpret_cast<uint32_t *>(L.part);
    u32 *spv = spk + MAX_SPECIAL_HP;
    uint8_t *mcode = reinterpret_cast<uint8_t *>(spk + 2 * MAX_SPECIAL_HP);
    int8_t *mpt = reinterpret_cast<int8_t *>(mcode + MAX_MOTIF);
    static_assert(2 * MAX_SPECIAL_HP * 4 + 2 * MAX_MOTIF <= PLay<NM>::MLA - PLay<NM>::PART, "setup tables fit the partials");
    if (tid < MAX_SPECIAL_HP) {
        const bool on = tid < n_sp;
        spk[tid] = on ? v_spk : 0xFFFFFFFFu;
        spv[tid] = on ? v_spv : INF16;
    }
    if (tid < MAX_MOTIF) {
        mcode[tid] = v_mc;
        mpt[tid] = v_mp;
    }

    // ---- refold restore: the loads of all three tables (8-byte vector loads into
    // registers), stored to LDS after the motif scan, so their HBM latency overlaps
    // it (round 6; the loop of dependent load -> store pairs cost ~20k cycles per
    // fold group).
    constexpr int CNM = ((NM - 4) * (NM - 3)) >> 1;
    constexpr int RS = (3 * (CNM >> 1) + NT - 1) / NT;   // loads per thread
    const int Crs = ((N - 4) * (N - 3)) >> 1, half = Crs >> 1;
    uint2 rsv[RS];
    constexpr int RC = (((CNM + 15) >> 4) + NT - 1) / NT;   // per-cell code loads per thread (uint4)
    const int C16 = (Crs + 15) >> 4;
    uint4 rcv[RC];
    u32 rod = 0, r5 = 0;   // the odd last cell of each table, q5's prefix
    if (incr) {
        const size_t Cs = size_t(ka.cells);
        const size_t gap = Cs - size_t(2 * half);   // from a table's last pair of cells to the next table
#pragma unroll
        for (int t = 0; t < RS; t++) {
            const int k = tid + t * NT;
            const int kk = k < 3 * half ? k : 0;
            // pair kk of the three tables' pairs: table kk / half, found by comparing (a
            // run-time division per load, and by zero at N <= 5, before)
            const size_t o = size_t(2 * kk) + (kk >= half ? gap : 0) + (kk >= 2 * half ? gap : 0);
            rsv[t] = gld(reinterpret_cast<const uint2 *>(inc.src + uint32_t(o)));
        }
#pragma unroll
        for (int t = 0; t < RC; t++) {
            const int k = tid + t * NT;
            rcv[t] = gld(inc.cc_src + uint32_t(k < C16 ? k : 0));
        }
        rod = gld(inc.src + uint32_t(min(tid, 2) * Cs + max(Crs - 1, 0)));
        r5 = gld(inc.src + uint32_t(3 * Cs + min(tid, N)));
    } else {
        const int C = ((N - 4) * (N - 3)) >> 1;
        for (int k = tid; k < C; k += NT) L.qm[k] = INF16;
    }
#ifdef ADX_STAMP
    const unsigned long long st_s1 = __builtin_amdgcn_s_memtime();   // setup tables stored, restore issued
#endif
    const bool constrained = block_or(L.flag, cst);
    const int mL = uni(gld(&XS->motif_len));
#ifdef ADX_STAMP
    const unsigned long long st_s2 = __builtin_amdgcn_s_memtime();   // sequence, constraints
#endif
    if ((mh0 || mh1) && mL > 0) {
        // fold_common.hpp motif_scan, open-coded: lanes = starts; the motif's positions in
        // chunks of 8 independent reads (one LDS round trip per chunk, not one per
        // position of the longest match)
        for (int o0 = 1 + wid * WAVE; o0 + mL - 1 <= N; o0 += NT) {
            const int o = o0 + lane;
            const bool in = o + mL - 1 <= N;
            bool ok = in;
            for (int k0 = 0; k0 < mL; k0 += 8) {
                uint32_t sb[8], mb[8];
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    sb[t] = L.S[min(o + k0 + t, N + 1)];
                    mb[t] = mcode[k0 + t];
                }
#pragma unroll
                for (int t = 0; t < 8; t++) ok = ok && (k0 + t >= mL || sb[t] == mb[t]);
                if (__ballot(ok) == 0) break;
            }
            if (in) L.mat[o] = ok ? 1 : 0;
        }
        __syncthreads();
        motif_constraints<NWV>(L, mpt, mL, N, wid, lane);
    }
#ifdef ADX_STAMP
    const unsigned long long st_s25 = __builtin_amdgcn_s_memtime();   // motif scan done
#endif
    if (incr) {   // the restore's stores (loads issued at the start)
        // qbm, qm and qm1 lie one table stride apart in LDS
        static_assert(PLay<NM>::QM - PLay<NM>::QBM == PLay<NM>::QM1 - PLay<NM>::QM, "one stride between the tables");
        const int gapl = int((PLay<NM>::QM - PLay<NM>::QBM) / 4) - 2 * half;
#pragma unroll
        for (int t = 0; t < RS; t++) {
            const int k = tid + t * NT;
            if (k < 3 * half) {
                const int o = 2 * k + (k >= half ? gapl : 0) + (k >= 2 * half ? gapl : 0);
                *reinterpret_cast<uint2 *>(L.qbm + o) = rsv[t];
            }
        }
        if ((Crs & 1) && tid < 3) (tid == 0 ? L.qbm : tid == 1 ? L.qm : L.qm1)[Crs - 1] = rod;
#pragma unroll
        for (int t = 0; t < RC; t++) {   // the codes (16 cells per store; the band's are recomputed)
            const int k = tid + t * NT;
            if (k < C16) reinterpret_cast<uint4 *>(L.cc)[k] = rcv[t];
        }
        if (tid <= m_lo - 2 && tid <= N) L.q5[tid] = r5;
    }
    // the per-cell pass's quarter-sets (below): diagonal d's band rows in sets of 16,
    // listed diagonal by diagonal in the split slots' space (free until the sweep)
    // by the waves of lane-sets 0, 1 of the diagonals: qtab[k] = d | first row << 8
    static_assert(NM - 4 <= 2 * WAVE, "the diagonals' quarter-set counts in two lane-sets");
    static_assert((NM - 4) + ((NM - 4) * (NM - 3) / 2 + 15) / 16 <= 6 * (NM + 2), "quarter-sets fit the split slots");
    u32 *qtab = L.mla;
    int tot = 0;  // quarter-sets
#pragma unroll
    for (int xs = 0; xs < 2; xs++) {
        const int d = 4 + xs * WAVE + lane;
        const int n = d <= N - 1 ? max(0, bd.chi(d) - bd.clo(d) + 1) : 0;
        const int q = (n + 15) >> 4;
        int v = q;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int t = __shfl_up(v, o, WAVE);
            if (lane >= o) v += t;
        }
        if (wid == xs)
            for (int c = 0; c < q; c++) qtab[tot + v - q + c] = u32(d) | (u32(bd.clo(d) + 16 * c) << 8);
        tot += __shfl(v, WAVE - 1, WAVE);
    }
    tot = uni(tot);
    __syncthreads();
    const u32 mx = u32(uni(int(__float_as_uint(gld(&XS->motif_extra)))));
    const u32 mextra = (mh0 ? (mx & 0xFFFFu) : 0x7FFFu) | (mh1 ? (mx & 0xFFFF0000u) : 0x7FFF0000u);
    if (tid == 0) q5_start(L, N);
#ifdef ADX_STAMP
    const unsigned long long st_s3 = __builtin_amdgcn_s_memtime();   // motif sites
#endif
    // ---- per-cell setup of the changed band (cell_pass above)
    for (int I0 = wid * 4; 4 * I0 < tot; I0 += NWV * 4)
        cell_pass(L, bd, lane, I0, qtab, tot, hpf, spk, spv, mL, mextra);
#ifdef ADX_STAMP
    const unsigned long long st_s35 = __builtin_amdgcn_s_memtime();   // this wave's cells (before the barrier)
#endif
    __syncthreads();
#ifdef ADX_STAMP
    const unsigned long long st_s4 = __builtin_amdgcn_s_memtime();   // per-cell pass
#endif
    // the partial, split and U slots start impossible (the setup used their space)
    for (int k = tid; k < 4 * 2 * NP; k += NT) L.part[k] = PINF;
    for (int k = tid; k < 6 * NP; k += NT) L.mla[k] = INF16;
    for (int k = tid; k < 4 * NP; k += NT) L.colmin[k] = INF16;
    __syncthreads();
#ifdef ADX_STAMP
    {
        const unsigned long long st_end = __builtin_amdgcn_s_memtime();
        sst[0] = st_end - st_setup0;
        sst[1] = st_s1 - st_setup0;
        sst[2] = st_s2 - st_s1;
        sst[3] = st_s25 - st_s2;
        sst[4] = st_s3 - st_s25;
        sst[5] = st_s4 - st_s3;
        sst[6] = st_s35 - st_s3;
    }
#endif
    return constrained;
}

// ---------------------------------------------------------------- the roles of a step
// L: the pairable cells of diagonals db, db+1 (ranks < P0 on db) and the B records of
// ranks < 64 into list slot sl (a step's B reads them two steps later: its first
// lane-set's records are loaded a step ahead, across the barrier)
__device__ __forceinline__ void build_list(const CP &L, const Band &bd, int lane, int db, int sl) {
    const int N = bd.N, NP2 = 2 * L.np;
    int base = 0, P0 = 0;
    for (int k = 0; k < 2; k++) {
        const int dn = db + k;
        if (k == 1) P0 = base;
        if (dn < 8 || dn > N - 1) continue;   // interior loops u >= 2 need spans >= 8
        const int lo = bd.clo(dn), hi = bd.chi(dn);
        const int Ln = lanesets(hi - lo + 1);
        for (int ls = 0; ls < Ln; ls++) {
            const int i = lo + ls * WAVE + lane;
            const bool pr = i <= hi && L.qbm[off(dn, N) + i - 1] != MARK16;
            const uint64_t m = __ballot(pr);
            const int rk = base + __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
            if (pr) L.cl[sl * NP2 + rk] = uint8_t(i);
            if (pr && rk < WAVE) {
                const int j = i + dn;
                const int oc = brec_code(L, i, j);
                const u32 mmo = L.dt[DT_MMI + oc];
                u32 *rr = L.rec + sl * 2 * WAVE + rk;
                rr[0] = brec_word(i, oc, L.up[i + 1], L.dn[j - 1]);
                // one half of each energy: two-word records (mfe_cells.hip: three words)
                rr[WAVE] = (mmo & 0xFFFFu) | (padd(L.ct[CT_ONEN + oc], mmo) << 16);
            }
            base += __popcll(m);
        }
    }
    if (lane == 0) L.cnt[sl] = P0 | (base << 16);
}
// A step's list counts (CP::cnt) and its first lane-set's B record, loaded at the top
// of the step before (issued with nothing to wait on: they complete under the
// step's first read batch); the records of the 4-lanes-per-cell mapping (lane &
// 15), the one of ~96 % of a refold's steps -- B reads its records itself when the
// step maps its lanes otherwise
__device__ __forceinline__ void load_list(const CP &L, int lane, int sl, int &PP, u32 &wd, u32 &mm) {
    PP = L.cnt[sl];
    const u32 *rr = L.rec + sl * 2 * WAVE + (lane & 15);
    wd = rr[0];
    mm = rr[WAVE];
}

// F's anchor and running values (the waves with a finalize lane-set)
struct FRun {
    int ab;                           // the anchor: lane 0 of lane-set 0 is row ab (0: not chosen yet)
    int pk;                           // the mode ab was chosen in: 1 packed (one wave, a cell per lane), 0 two cells per lane
    int fd;                           // the step the values below stand for (0, or a step this wave sat out: none)
    int oE0, oE1, oS1, oS2, oS3;      // uniform: off() of spans e0, e1, e0-1, e0-2, e0-3
    uint32_t mS, mM;                  // uniform: split slots e0 % 6, (e0 + 4) % 6 (bytes)
    uint32_t cW;                      // uniform: U slot e0 & 3 (bytes; the partials': twice that)
    int fI;                           // per lane: the row,
    uint32_t fSi, fSi1, fUi, fUi1;    //   S[i], S[i+1], up[i], up[i+1],
    uint32_t fRq;                     //   the address of qm(i, i + 4) less 4 words,
    uint32_t fJ4, fSj, fQ1;           //   4 jA, the addresses of S[jA - 1] and qm1(i, jA - 1)
                                      //   (packed: of the lane's own column j = jA | jA + 1)
    uint32_t fH;                      //   packed: the lane's half as a ring-slot stride (0 | NP words, bytes)
};

// F packed (the finalize wave, a window of at most 32 rows): the cells of one
// step side by side.  Lane l is row ab + (l & 31); lanes 0..31 finalize the
// span-e0 cell (i, jA) of their row, lanes 32..63 the span-e1 cell (i, jA + 1) of
// the same row, each from one read batch of its own cell's terms.  The per-lane
// running values are those of finalize() taken at the lane's own column j (the
// slow path adds the half to jA); the uniform ones are shared with the
// two-cells-per-lane mode, and a half picks its spans' offsets from them.  Two
// values cross the halves: qm1(i, jA), the upper half's qm1 predecessor, comes
// from lane l - 32 in one v_permlane32_swap once the lower half has it, and
// U(i + 1, jA + 1) from lower-half lane (l & 31) + 1 through F's ds_bpermute.
// One lane-set, so no overlap lane: every lane of the window owns its cell.  The
// window's last row is row R (no span-e1 cell) or the ghost (its U is the
// restored qm) as in finalize(), and it sits on lane lr - ab <= 31, so the
// upper half's last row never uses the neighbour it does not have (lane 32, or a
// masked lane).  q1P, q1: the addresses of qm1(i, j - 1) and qm1(i, j).
// (tests/test_finalize_packed_model.py restates the mapping and the addresses)
template <int NM>
__device__ __forceinline__ void finalize_packed(const CP &L, const FRun &f, const BUni &U, int N, int e0, int lane,
                                                int mloF, int mhiF, u32 mlclosing, u32 mlbase, uint32_t q1P,
                                                uint32_t q1 PSTAMP_PARAMS) {
    constexpr uint32_t NP4 = uint32_t(NM + 2) * 4u;
    const uint32_t aq = U.aq, ac = U.ac;
    const bool hB = lane >= 32;
    const int i = f.fI;
    const uint32_t i4 = uint32_t(i) * 4u, iH = i4 + f.fH;
    const int e = e0 + (hB ? 1 : 0);                 // the lane's span
    const int j = int(f.fJ4 >> 2);                   // and column, i + e
    const int oE = hB ? f.oE1 : f.oE0;               // off() of spans e, e-2, e-3
    const int o2 = hB ? f.oS1 : f.oS2, o3 = hB ? f.oS2 : f.oS3;
    const bool cell = j <= N;                        // row R has no span-e1 cell
    const bool ghost = i == mhiF + 3;
    const uint32_t qX = (aq - 4u) + uint32_t(oE) * 4u + i4;
    const uint32_t pA = (lds_addr(L.part) + 2u * f.cW) + iH + f.fH;   // slot e & 3, both halves
    const uint32_t uW = (lds_addr(L.colmin) + f.cW) + f.fH + f.fJ4;   // U(.., j) of span e
    const uint32_t gq = f.fRq + (f.fJ4 - i4);                         // qm(i, j)
    u32 init, cce, st, pq, ml, sp, up, p0, p1, v2, c2, v3, c3, v3b, c3b, gv;
    uint32_t sjm, sj, uj, djm;
    const uint32_t si = f.fSi, si1 = f.fSi1, ui = f.fUi, ui1 = f.fUi1;
    {
        const uint32_t mA = (lds_addr(L.mla) + f.mM + 4u) + iH;   // span e-2, row i + 1
        const uint32_t sA = (lds_addr(L.mla) + f.mS) + iH;        // slot e % 6
        // U(i + 1, jA) of span e0-1 (the lower half's; the upper half takes its U across the halves
        // and reads the next column of the same slot for nothing)
        const uint32_t uA = (lds_addr(L.colmin) + 3u * NP4 - f.cW) + f.fJ4;
        asm volatile(
            "ds_read_b32 %[init], %[qX]\n"
            "ds_read_u8 %[cce], %[kX]\n"
            "ds_read_b32 %[st], %[q1]\n"
            "ds_read_b32 %[pq], %[q1P]\n"
            "ds_read_b32 %[ml], %[mA]\n"
            "ds_read_b32 %[sp], %[sA]\n"
            "ds_read_b32 %[up], %[uA]\n"
            "ds_read_b32 %[p0], %[pA]\n"
            "ds_read_b32 %[p1], %[pA] offset:%[pst]\n"
            "ds_read_b32 %[v2], %[q2]\n"
            "ds_read_b32 %[v3], %[q3]\n"
            "ds_read_b32 %[v3b], %[q3] offset:4\n"
            "ds_read_u8 %[c2], %[k2]\n"
            "ds_read_u8 %[c3], %[k3]\n"
            "ds_read_u8 %[c3b], %[k3] offset:1\n"
            // S, up, dn lie NP bytes apart (the carve): one address, j - 1 in S
            "ds_read_u8 %[sjm], %[aSj] offset:0\n"
            "ds_read_u8 %[sj], %[aSj] offset:1\n"
            "ds_read_u8 %[uj], %[aSj] offset:%[ou]\n"
            "ds_read_u8 %[djm], %[aSj] offset:%[od]\n"
            "ds_read_b32 %[gv], %[gq]\n"
            "s_waitcnt lgkmcnt(0)"
            : [init] "=&v"(init), [cce] "=&v"(cce), [st] "=&v"(st), [pq] "=&v"(pq), [ml] "=&v"(ml), [sp] "=&v"(sp),
              [up] "=&v"(up), [p0] "=&v"(p0), [p1] "=&v"(p1), [v2] "=&v"(v2), [v3] "=&v"(v3), [v3b] "=&v"(v3b),
              [c2] "=&v"(c2), [c3] "=&v"(c3), [c3b] "=&v"(c3b), [sjm] "=&v"(sjm), [sj] "=&v"(sj), [uj] "=&v"(uj),
              [djm] "=&v"(djm), [gv] "=&v"(gv)
            : [qX] "v"(qX), [kX] "v"((ac - 1u) + uint32_t(oE) + uint32_t(i)), [q1] "v"(q1), [q1P] "v"(q1P), [mA] "v"(mA),
              [sA] "v"(sA), [uA] "v"(uA), [pA] "v"(pA), [pst] "i"(NP4), [q2] "v"(aq + uint32_t(o2) * 4u + i4),
              [q3] "v"(aq + uint32_t(o3) * 4u + i4), [k2] "v"(ac + uint32_t(o2) + uint32_t(i)),
              [k3] "v"(ac + uint32_t(o3) + uint32_t(i)), [aSj] "v"(f.fSj), [ou] "i"(NM + 2 + 1),
              [od] "i"(2 * (NM + 2)), [gq] "v"(gq)
            : "memory");
    }
#ifdef ADX_STAMP_F
    PSTAMP(11);   // F: the read batch
#endif
    const int ty = ptype(si, sj), t8 = ty * 8;
    auto stk = [&](u32 v, u32 c) {   // inner pair with code c closing a stack with the cell's type
        return padd(v, padd(L.ct[CT_INVMM + c], L.ct[CT_STK + t8 + ((int(c) * 41) >> 10)]));
    };
    // (i, j): stack inner (i+1, j-1) span e-2 [v2]; bulges (0,1) inner (i+1, j-2) [v3],
    // (1,0) inner (i+2, j-1) [v3b], span e-3.  The lookups stay behind their conditions:
    // taking all eight table entries in one round trip, needed or not, measured -0.3 %
    // (profiles/fpack_ab.txt)
    u32 iX = e >= 6 ? stk(v2, c2) : INF16;
    if (e0 >= 6) {   // (e0 = 4: e < 7 on both halves)
        const bool b7 = e >= 7;
        iX = pmin(iX, b7 && djm >= 1 ? padd(stk(v3, c3), U.fs1) : INF16);
        iX = pmin(iX, b7 && ui1 >= 1 ? padd(stk(v3b, c3b), U.fs1) : INF16);
    }
    const u32 mlcl = padd(mlclosing, L.dt[DT_MLS + rtype(ty) * 25 + sjm * 5 + si1]);
    const u32 mmi = L.dt[DT_MMI + cce];
    // the band's rows of the lane's span (Band::clo .. chi: i >= m_lo - 1 - e)
    const bool in = cell && j >= mloF - 1 && i <= mhiF + 1;
    auto st32 = [](uint32_t a, u32 v) { *lds_at<u32>(a) = v; };   // the batch's addresses serve the stores
    const bool pairable = init != MARK16;
    u32 c = pmin(init, pack2(int(p0), int(p1)));
    c = pmin(c, iX);
    c = pfin(pmin(c, padd(ml, mlcl)));
    if (in && pairable) st32(qX, pfin(padd(c, mmi)));
    const u32 cs = pairable ? padd(c, st) : INF16;
    const bool pv = e >= 5 && uj >= 1;
    // qm1 = min(c + stem, qm1(i, j - 1) + MLbase); restored outside the band
    auto m1of = [&](u32 p) { return in ? pfin(pmin(cs, pv ? padd(p, mlbase) : INF16)) : st; };
    u32 m1 = m1of(pq);
    // the upper half's predecessor (i, jA) is the lower half's cell of the same row: the swap
    // leaves pq in lanes 0..31 and puts lane l - 32's m1 into lanes 32..63
    const auto sw = __builtin_amdgcn_permlane32_swap(pq, m1, false, false);
    m1 = m1of(u32(sw[0]));
    if (in) st32(q1, m1);
#ifdef ADX_STAMP_F
    PSTAMP(12);   // F: the cells' terms
#endif
    auto uof = [&](u32 below) { return ghost ? gv : (ui >= 1 ? pmin(m1, padd(below, mlbase)) : m1); };
    // U of row i+1 in column jA+1 (span e0) is the lower half's value of the next row
    const u32 UA1 = u32(__builtin_amdgcn_ds_bpermute(((lane & 31) + 1) * 4, int(uof(up))));
    const u32 Uf = uof(hB ? UA1 : up);
    if (cell) {
        st32(uW, Uf);
        st32(pA, u32(PINF));
        st32(pA + NP4, u32(PINF));
        if (e <= N - 3 && j >= mloF - 2 && i <= mhiF + 2)   // Band::qlo(e) .. qhi(e)
            st32(gq, pfin(pmin(e >= 9 ? sp : INF16, Uf)));
    }
#ifdef ADX_STAMP_F
    PSTAMP(13);   // F: U, the stores
#endif
}

// F: finalize e0 = d-2 and e1 = d-1 on lane-set fls.  mloF, mhiF: the changed hull (a
// fold from scratch is a refold whose hull clamps nowhere).  Lanes = rows i, from
// row fr to row lr.  A fold from scratch: all rows.  A refold: the rows whose
// qm it rewrites (Band::qlo(e1) .. qhi(e0); the qbm / qm1 band lies inside) and one
// ghost row m_hi + 3 above them, where the span has it.  The ghost writes no
// table cell: it hands the restored qm of its two cells down as their unpaired
// parts U.  That is exact: qm(r, j) = min(split(r, j), U(r, j)), and every split
// of (r, j) plus the MLbase of the unpaired rows below r is a split of the row
// that takes it (same right part, left part qm one row longer), so the band's
// qm = min(split, U) is the same with either (tests/test_qm_boundary.py).
// Rows above the ghost only carried U and are not run.  A lane-set spans 64
// rows, consecutive lane-sets overlap by one row (lane 63 recomputes the next
// set's first row for its U and writes nothing), so no value crosses waves;
// the window's last row is row R (no cell of span e1) or the ghost, so the
// last lane needs no neighbour.
//
// Lanes keep their rows: lane l of lane-set fls is row ab + 63 fls + l while
// the anchor ab holds, and is masked off (EXEC) outside the step's window
// [fr, lr].  The window only moves down (fr, lr never grow), so the anchor is
// the lowest row from which the lane-sets still reach lr: max(1, lr - 63) for a
// window of one lane-set, max(1, lr - 126) for a longer one, chosen at the first
// step and again only when fr falls below it -- never in a fold from scratch
// (fr = 1), at most once in a one-position refold (changed row >= 62).  Between
// re-anchors every address is last step's plus a delta: the spans' cell offsets
// and the ring slots are uniform shift registers, the lane's column and its qm1
// column base advance by adds, its row's bytes and qm base stay
// (tests/test_finalize_anchor_model.py restates all of it).
//
// The mode is chosen with the anchor: a window that fits a half-wave
// (lr - fr <= 31) runs packed on the finalize wave (finalize_packed above: anchor
// max(1, lr - 31), lane-set 1 does not exist), any other as described here.  The
// rule is a function of (fr, lr, the previous anchor and mode) alone: re-anchor
// when there is no anchor, when fr falls below it or when the fit differs from
// the mode, so a change of mode goes through the slow path like any re-anchor.
// The window grows by two rows a step until it clamps and shrinks with R: at
// most two changes a sweep after the first choice (packed, two cells per lane,
// packed).  Both F waves evaluate the rule; the uniform running values serve
// both modes.
template <int NM, int fls>
__device__ __forceinline__ void finalize(const CP &L, FRun &f, const BUni &U, int N, int d, int lane, int mloF,
                                         int mhiF, u32 mlclosing, u32 mlbase PSTAMP_PARAMS) {
    static_assert(NM - 4 <= 2 * WAVE - 1, "two overlapping lane-sets reach every row from row 1");
    static_assert(PLay<NM>::NP == NM + 2 && 4 * (NM + 2) * 4 < 65536, "slot strides as ds offsets");
    const uint32_t aqm = lds_addr(L.qm), aqm1 = lds_addr(L.qm1);
    const int e0 = d - 2, e1 = d - 1;
    const int R = N - e0;                                   // rows of span e0 (e1: R - 1)
    const int fr = max(1, mloF - 2 - e1);                   // Band::qlo(e1)
    const int lr = min(R, mhiF + 3);
    const int fit = lr - fr <= 31 ? 1 : 0;                    // the window fits a half-wave: packed
    if (e0 <= N - 1 && (f.ab == 0 || fr < f.ab || fit != f.pk)) {   // (re-)anchor: both F waves alike
        f.pk = fit;
        f.ab = max(1, lr - (fit ? 31 : (lr - fr < 64 ? 63 : 126)));
        f.fd = 0;
    }
    if (e0 <= N - 1 && (fls == 0 || lr - f.ab > 63)) {        // lane-set 1: only past row ab + 63 (never packed)
        __builtin_amdgcn_s_setprio(PRIO_ROLE);
        constexpr uint32_t NP4 = uint32_t(NM + 2) * 4u;      // a ring slot, a partial half (bytes)
        const uint32_t aq = U.aq, ac = U.ac, aS = lds_addr(L.S);
        if (fls == 1 || f.fd != d) {   // the slow path: the closed forms at (ab, d); lane-set 1 (a block
                                     // wave, a few steps of a wide refold) keeps no state but ab
            const bool pk = fls == 0 && f.pk != 0;
            const int hB = pk && lane >= 32 ? 1 : 0;           // packed: the upper half's cells are one span on
            f.fI = f.ab + (pk ? (lane & 31) : fls * 63 + lane);
            f.fH = hB ? NP4 : 0u;
            const int ic = min(f.fI, N);                       // rows past N are never active
            f.fSi = L.S[ic], f.fSi1 = L.S[ic + 1], f.fUi = L.up[ic], f.fUi1 = L.up[ic + 1];
            f.fRq = aqm + uint32_t(rowb(f.fI, N) - 4) * 4u;
            const int jA = f.fI + e0 + hB;
            f.fJ4 = uint32_t(jA) * 4u;
            f.fSj = aS + uint32_t(jA - 1);
            f.fQ1 = aqm1 + uint32_t(colb(jA - 1) + f.fI - 1) * 4u;
            // inner cells of the stack / bulge-1 shapes: spans e0-1, e0-2, e0-3 (the
            // impossible span 3 stands in for the ones no shape reads yet)
            f.oE0 = off(e0, N), f.oE1 = off(e1, N);
            f.oS1 = off(max(e0 - 1, 3), N), f.oS2 = off(max(e0 - 2, 3), N), f.oS3 = off(max(e0 - 3, 3), N);
            f.mS = uint32_t(e0 % 6) * NP4, f.mM = uint32_t((e0 + 4) % 6) * NP4;
            f.cW = uint32_t(e0 & 3) * NP4;
            f.fd = d;
        }
        const int i = f.fI;
        const uint32_t i4 = uint32_t(i) * 4u;
        const uint32_t q1P = f.fQ1, q1A = q1P + (f.fJ4 - 20u), q1B = q1A + (f.fJ4 - 16u);   // colb(j+1) - colb(j) = j - 4
        if (i >= fr && i <= lr) {
        bool pk = false;
        if constexpr (fls == 0) pk = f.pk != 0;
        if (pk) {
            finalize_packed<NM>(L, f, U, N, e0, lane, mloF, mhiF, mlclosing, mlbase, q1P, q1A PSTAMP_ARGS);
        } else {
        const bool own = lane < 63 || fls == 1 || lr - f.ab <= 63;   // the overlap lane writes nothing
        const bool rowB = i <= R - 1;
        const bool ghost = i == mhiF + 3;
        const uint32_t qA = (aq + uint32_t(f.oE0 - 1) * 4u) + i4, qB = (aq + uint32_t(f.oE1 - 1) * 4u) + i4;
        const uint32_t pA = (lds_addr(L.part) + 2u * f.cW) + i4;       // slot e0 & 3; e1 & 3 is the next
        const uint32_t uW = (lds_addr(L.colmin) + f.cW) + f.fJ4;         // U(.., jA) of span e0; e1: the next slot
        const uint32_t gq = f.fRq + uint32_t(e0) * 4u;                 // qm(i, jA), qm(i, jA + 1)
        u32 initA, cceA, stA, pqA, mlA, spA, upA, a0, a1, vS3, cS3, vS3b, cS3b, vS2, cS2, vS2b, cS2b, vS1, cS1;
        u32 initB, cceB, stB, mlB, spB, b0, b1, gqA, gqB;
        uint32_t sjm, sj, sjp, ujA, ujB, djm, dj;
        const uint32_t si = f.fSi, si1 = f.fSi1, ui = f.fUi, ui1 = f.fUi1;
        {
            const uint32_t mA = (lds_addr(L.mla) + f.mM + 4u) + i4;   // span e0-2 (slot (e0 + 4) % 6), row i + 1; e1-2: the next slot
            const uint32_t sA = (lds_addr(L.mla) + f.mS) + i4;        // slot e0 % 6; e1 % 6 is the next
            const uint32_t uA = (lds_addr(L.colmin) + 3u * NP4 - f.cW) + f.fJ4;   // span e0-1: slot (e0 + 3) & 3
            asm volatile(
                "ds_read_b32 %[initA], %[qA]\n"
                "ds_read_u8 %[cceA], %[kA]\n"
                "ds_read_b32 %[stA], %[q1A]\n"
                "ds_read_b32 %[pqA], %[q1P]\n"
                "ds_read_b32 %[mlA], %[mA]\n"
                "ds_read_b32 %[spA], %[sA]\n"
                "ds_read_b32 %[upA], %[uA]\n"
                "ds_read_b32 %[a0], %[pA]\n"
                "ds_read_b32 %[a1], %[pA] offset:%[pst]\n"
                "ds_read_b32 %[initB], %[qB]\n"
                "ds_read_u8 %[cceB], %[kB]\n"
                "ds_read_b32 %[stB], %[q1B]\n"
                "ds_read_b32 %[mlB], %[mA] offset:%[pst]\n"
                "ds_read_b32 %[spB], %[sA] offset:%[pst]\n"
                "ds_read_b32 %[b0], %[pA] offset:%[pst2]\n"
                "ds_read_b32 %[b1], %[pA] offset:%[pst3]\n"
                "ds_read_b32 %[vS3], %[q3]\n"
                "ds_read_b32 %[vS3b], %[q3] offset:4\n"
                "ds_read_b32 %[vS2], %[q2]\n"
                "ds_read_b32 %[vS2b], %[q2] offset:4\n"
                "ds_read_b32 %[vS1], %[q1]\n"
                "ds_read_u8 %[cS3], %[k3]\n"
                "ds_read_u8 %[cS3b], %[k3] offset:1\n"
                "ds_read_u8 %[cS2], %[k2]\n"
                "ds_read_u8 %[cS2b], %[k2] offset:1\n"
                "ds_read_u8 %[cS1], %[k1]\n"
                // S, up, dn lie NP bytes apart (the carve): one address, jA - 1 in S
                "ds_read_u8 %[sjm], %[aSj] offset:0\n"
                "ds_read_u8 %[sj], %[aSj] offset:1\n"
                "ds_read_u8 %[sjp], %[aSj] offset:2\n"
                "ds_read_u8 %[ujA], %[aSj] offset:%[ou0]\n"
                "ds_read_u8 %[ujB], %[aSj] offset:%[ou1]\n"
                "ds_read_u8 %[djm], %[aSj] offset:%[od0]\n"
                "ds_read_u8 %[dj], %[aSj] offset:%[od1]\n"
                "ds_read_b32 %[gqA], %[gq]\n"
                "ds_read_b32 %[gqB], %[gq] offset:4\n"
                "s_waitcnt lgkmcnt(0)"
                : [initA] "=&v"(initA), [cceA] "=&v"(cceA), [stA] "=&v"(stA), [pqA] "=&v"(pqA), [mlA] "=&v"(mlA),
                  [spA] "=&v"(spA), [upA] "=&v"(upA), [a0] "=&v"(a0), [a1] "=&v"(a1), [initB] "=&v"(initB),
                  [cceB] "=&v"(cceB), [stB] "=&v"(stB), [mlB] "=&v"(mlB), [spB] "=&v"(spB), [b0] "=&v"(b0),
                  [b1] "=&v"(b1), [vS3] "=&v"(vS3), [vS3b] "=&v"(vS3b), [vS2] "=&v"(vS2), [vS2b] "=&v"(vS2b),
                  [vS1] "=&v"(vS1), [cS3] "=&v"(cS3), [cS3b] "=&v"(cS3b), [cS2] "=&v"(cS2), [cS2b] "=&v"(cS2b),
                  [cS1] "=&v"(cS1), [sjm] "=&v"(sjm), [sj] "=&v"(sj), [sjp] "=&v"(sjp), [ujA] "=&v"(ujA),
                  [ujB] "=&v"(ujB), [djm] "=&v"(djm), [dj] "=&v"(dj), [gqA] "=&v"(gqA), [gqB] "=&v"(gqB)
                : [qA] "v"(qA), [kA] "v"((ac + uint32_t(f.oE0 - 1)) + uint32_t(i)), [q1A] "v"(q1A), [q1P] "v"(q1P),
                  [mA] "v"(mA), [sA] "v"(sA), [uA] "v"(uA), [pA] "v"(pA), [pst] "i"(NP4), [pst2] "i"(2 * NP4),
                  [pst3] "i"(3 * NP4), [qB] "v"(qB), [kB] "v"((ac + uint32_t(f.oE1 - 1)) + uint32_t(i)), [q1B] "v"(q1B),
                  [q3] "v"((aq + uint32_t(f.oS3) * 4u) + i4), [q2] "v"((aq + uint32_t(f.oS2) * 4u) + i4),
                  [q1] "v"((aq + uint32_t(f.oS1) * 4u) + i4), [k3] "v"((ac + uint32_t(f.oS3)) + uint32_t(i)),
                  [k2] "v"((ac + uint32_t(f.oS2)) + uint32_t(i)), [k1] "v"((ac + uint32_t(f.oS1)) + uint32_t(i)),
                  [aSj] "v"(f.fSj), [ou0] "i"(NM + 2 + 1), [ou1] "i"(NM + 2 + 2), [od0] "i"(2 * (NM + 2)),
                  [od1] "i"(2 * (NM + 2) + 1), [gq] "v"(gq)
                : "memory");
        }
#ifdef ADX_STAMP_F
        PSTAMP(11);   // F: the read batch
#endif
        static_assert(NM + 2 == PLay<NM>::NP, "partial halves are NP words apart");
        // the loop-correction factors of the stack / bulge-1 shapes and the cells' own terms
        const int tyA = ptype(si, sj), tyB = ptype(si, sjp);
        const int t8A = tyA * 8, t8B = tyB * 8;
        auto stk = [&](u32 v, u32 c, int t8) {   // inner pair with code c closing a stack with type t8/8
            return padd(v, padd(L.ct[CT_INVMM + c], L.ct[CT_STK + t8 + ((int(c) * 41) >> 10)]));
        };
        // A = (i, jA): stack inner (i+1, jA-1) span e0-2 [vS2]; bulges (0,1) inner
        // (i+1, jA-2) [vS3], (1,0) inner (i+2, jA-1) [vS3b], span e0-3.
        // B = (i, jA+1): stack inner (i+1, jA) span e0-1 [vS1]; bulges (0,1) inner
        // (i+1, jA-1) [vS2], (1,0) inner (i+2, jA) [vS2b], span e0-2.
        u32 iA = INF16, iB = INF16;
        if (e0 >= 6) iA = stk(vS2, cS2, t8A);
        if (e0 >= 7) {
            iA = pmin(iA, djm >= 1 ? padd(stk(vS3, cS3, t8A), U.fs1) : INF16);
            iA = pmin(iA, ui1 >= 1 ? padd(stk(vS3b, cS3b, t8A), U.fs1) : INF16);
        }
        if (e1 >= 6) iB = stk(vS1, cS1, t8B);
        if (e1 >= 7) {
            iB = pmin(iB, dj >= 1 ? padd(stk(vS2, cS2, t8B), U.fs1) : INF16);
            iB = pmin(iB, ui1 >= 1 ? padd(stk(vS2b, cS2b, t8B), U.fs1) : INF16);
        }
        const u32 mlclA = padd(mlclosing, L.dt[DT_MLS + rtype(tyA) * 25 + sjm * 5 + si1]);
        const u32 mlclB = padd(mlclosing, L.dt[DT_MLS + rtype(tyB) * 25 + sj * 5 + si1]);
        const u32 mmiA = L.dt[DT_MMI + cceA], mmiB = L.dt[DT_MMI + cceB];
        // the band's rows of the two spans (Band::clo .. chi; the window's rows have i <= R)
        const bool inA = i >= mloF - 1 - e0 && i <= mhiF + 1;
        const bool inB = rowB && e1 <= N - 1 && i >= mloF - 1 - e1 && i <= mhiF + 1;
        auto st32 = [](uint32_t a, u32 v) { *lds_at<u32>(a) = v; };   // the batch's addresses serve the stores
        // cell A
        u32 m1A = stA;   // restored qm1 outside the band
        if (inA) {
            const u32 prev = (e0 >= 5 && ujA >= 1) ? padd(pqA, mlbase) : INF16;
            u32 f1 = prev;
            if (initA != MARK16) {
                u32 c = pmin(initA, pack2(int(a0), int(a1)));
                c = pmin(c, iA);
                c = pfin(pmin(c, padd(mlA, mlclA)));
                if (own) st32(qA, pfin(padd(c, mmiA)));
                f1 = pmin(padd(c, stA), prev);
            }
            m1A = pfin(f1);
            if (own) st32(q1A, m1A);
        }
        const u32 UA = ghost ? gqA : (ui >= 1 ? pmin(m1A, padd(upA, mlbase)) : m1A);
        // cell B (its qm1 predecessor (i, jA) is cell A of this lane)
        u32 m1B = stB;
        if (inB) {
            const u32 prev = (e1 >= 5 && ujB >= 1) ? padd(m1A, mlbase) : INF16;
            u32 f1 = prev;
            if (initB != MARK16) {
                u32 c = pmin(initB, pack2(int(b0), int(b1)));
                c = pmin(c, iB);
                c = pfin(pmin(c, padd(mlB, mlclB)));
                if (own) st32(qB, pfin(padd(c, mmiB)));
                f1 = pmin(padd(c, stB), prev);
            }
            m1B = pfin(f1);
            if (own) st32(q1B, m1B);
        }
#ifdef ADX_STAMP_F
        PSTAMP(12);   // F: the cells' terms
#endif
        // U of row i+1 in column jA+1 (span e0) is the next lane's cell A (a window
        // row below lr has its neighbour in the window: both lanes are on)
        const u32 UA1 = u32(__builtin_amdgcn_ds_bpermute((lane + 1) * 4, int(UA)));
        const u32 UB = ghost ? gqB : (ui >= 1 ? pmin(m1B, padd(UA1, mlbase)) : m1B);
        if (own) {
            st32(uW, UA);
            st32(pA, u32(PINF));
            st32(pA + NP4, u32(PINF));
            if (e0 <= N - 3 && i >= mloF - 2 - e0 && i <= min(R, mhiF + 2))   // Band::qlo(e0) .. qhi(e0)
                st32(gq, pfin(pmin(e0 >= 9 ? spA : INF16, UA)));
        }
        if (own && rowB && e1 <= N - 1) {
            st32(uW + NP4 + 4u, UB);
            st32(pA + 2u * NP4, u32(PINF));
            st32(pA + 3u * NP4, u32(PINF));
            if (e1 <= N - 3 && i >= mloF - 2 - e1 && i <= min(R - 1, mhiF + 2))   // Band::qlo(e1) .. qhi(e1)
                st32(gq + 4u, pfin(pmin(e1 >= 9 ? spB : INF16, UB)));
        }
#ifdef ADX_STAMP_F
        PSTAMP(13);   // F: U, the stores
#endif
        }
        }
#ifdef ADX_STAMP_F
        {   // the sub-phase sums were advanced by the window's lanes only: every lane
            // (lane 0 reports) takes them from the first lane of the window
            const uint64_t on = __ballot(i >= fr && i <= lr);
            if (on != 0) {
                const int src = __ffsll((long long)on) - 1;
                auto from = [&](unsigned long long v) {
                    const uint32_t lo = __builtin_amdgcn_readlane(uint32_t(v), src);
                    const uint32_t hi = __builtin_amdgcn_readlane(uint32_t(v >> 32), src);
                    return (unsigned long long)lo | ((unsigned long long)hi << 32);
                };
                st_acc[11] = from(st_acc[11]), st_acc[12] = from(st_acc[12]), st_acc[13] = from(st_acc[13]);
                st_last = from(st_last);
            }
        }
#endif
        // the running values of the next step
        if constexpr (fls == 0) {
        f.fQ1 = q1B;                       // qm1(i, jA + 1): the predecessor column of step d + 2
        f.fJ4 += 8u, f.fSj += 2u;
        f.oS3 = f.oS1, f.oS2 = f.oE0, f.oS1 = f.oE1;
        f.oE0 = f.oE1 + (N - e1), f.oE1 = f.oE0 + (N - e1 - 1);   // off(e + 1) = off(e) + N - e
        f.mM = f.mS, f.mS = f.mS == 4u * NP4 ? 0u : f.mS + 2u * NP4;
        f.cW ^= 2u * NP4;
        f.fd = d + 2;
        }
        __builtin_amdgcn_s_setprio(0);
    }
}

// log2 slices (lanes) per cell of a lane-set over P cells
__device__ __forceinline__ int slices(int P) { return P <= 16 ? 2 : (P <= 32 ? 1 : 0); }

// B: interior-loop partials (u >= 2) of diagonals d and d+1.
// Lanes = the pairable cells of both (listed last step: ranks < P0 on d,
// the rest on d+1); a lane of d+1 reads its inner cells at
// off(d - 2 - u) + i + (N - d + 2 + u), which the blocks add per lane (hb).
// cPP, cwd, cmm: load_list of this step; blk: the wave's block; E: the 1x1 .. 2x2 energies by code pair
template <int blk>
__device__ __forceinline__ void block_partials(const CP &L, const uint16_t *E, BUni &U, int d, int lane, int sl, int cPP,
                                               u32 cwd, u32 cmm, bool constrained, u32 tauE, u32 fsm5 PSTAMP_PARAMS) {
    const int N = U.N, NP = L.np, NP2 = 2 * NP;
    const uint32_t ae4 = lds_addr(L.e4);
    if (d + 1 >= 8 && d <= N - 1) {
        const int P0 = uni(cPP & 0xFFFF), P = uni(cPP >> 16);
        const int sh = slices(P);
        const int cwl = 6 - sh;
        const int Lb = (P + (1 << cwl) - 1) >> cwl;
        const int r = lane >> cwl;
        U.d = d;
        U.umax = d - 5 < 30 ? d - 5 : 30;   // d+1's loop sizes; d's last one reads the impossible span 3
        for (int ls = 0; ls < Lb && blk < MFE_NBLK; ls++) {
            const int idx = (ls << cwl) + (lane & ((1 << cwl) - 1));
            if (idx < P) {
                const int hb = idx >= P0 ? 1 : 0;   // hb, dd: this kernel's two diagonals per lane-set
                const int dd = d + hb;
                BRec c;
                if (ls == 0 && sh == 2) {   // loaded a step ahead
                    c = brec_unpack(cwd, lo2(cmm), hi2(cmm));
                } else if (idx < WAVE) {
                    const u32 *rr = L.rec + sl * 2 * WAVE + idx;
                    c = brec_unpack(rr[0], lo2(rr[WAVE]), hi2(rr[WAVE]));
                } else {
                    const int i = L.cl[sl * NP2 + idx];
                    c = brec_of(L, i, i + dd);
                }
                const int i = c.i, oc = c.oc, type = (oc * 41) >> 10;
                const int uml = dd - 6 < 30 ? dd - 6 : 30;   // this lane's loop sizes
                BCell C;
                C.i = i + hb * (N - d + 2);
                C.hb = hb;
                C.ty8 = type * 8;
                bcell_slice(C, r, sh, ae4);
                C.A = c.A;
                C.B = c.B;
                const u32 tau = type > 2 ? tauE : 0u;
                // the loop sizes' table energies only on the wave whose block reads them
                // (bits of a literal: a runtime-indexed table would be a scalar load;
                // per block in mfe_cells.hip)
                auto has = [&](unsigned bits) { return ((bits >> (sh * 8 + blk)) & 1u) != 0; };
                C.m23f = has(size_bits(5)) ? padd(L.ct[CT_M23O + oc], fsm5) : INF16;
                C.t11 = C.t12 = C.t21 = C.t22 = INF16;
                bcell_tables(C, L, E, N, dd, i, oc, uml, has(size_bits(2)), has(size_bits(3)), has(size_bits(4)));
                Acc a{INF16, INF16, INF16, INF16, INF16, INF16};
                const bool mk = constrained && __ballot(C.A < uml || C.B < uml) != 0;
                U.mk = mk;
                PSTAMP(9);
                if (sh == 2) mfe_block_s4(blk, U, C, a);
                else if (sh == 1) mfe_block_s2(blk, U, C, a);
                else mfe_block(blk, U, C, a);
                PSTAMP(10);
                const u32 acc = acc_fold(a, C, sh, c.mmo, c.mo, tau);
                if (r == 0) {   // by row, the block waves' minima meet in atomics (mfe_cells.hip: a slot per block)
                    int *pp = L.part + (dd & 3) * 2 * NP + i;
                    atomicMin(pp, sext_lo(acc));
                    atomicMin(pp + NP, sext_hi(acc));
                }
            }
        }
    }
}

// 2 NR reads of a split-point chunk from t0 on (NR = 16, 8, 4: the chunk shapes are
// uniform) in one batch, folded into sp0 / sp1
template <int NR>
__device__ __forceinline__ void split_chunk(const CP &L, int N, int i, int j, int Tt, int t0, u32 &sp0, u32 &sp1) {
    const uint32_t aqm = lds_addr(L.qm), aqm1 = lds_addr(L.qm1);
    u32 av[NR], rv[NR];
    const uint32_t pa = aqm1 + uint32_t(colb(j) + i - 1 + t0) * 4u;
    const uint32_t pr = aqm + uint32_t(rowb(i, N) - 5 + t0) * 4u;
    if constexpr (NR == 16) {
        asm volatile(
                "ds_read_b32 %0, %32 offset:0\n"
                "ds_read_b32 %1, %32 offset:4\n"
                "ds_read_b32 %2, %32 offset:8\n"
                "ds_read_b32 %3, %32 offset:12\n"
                "ds_read_b32 %4, %32 offset:16\n"
                "ds_read_b32 %5, %32 offset:20\n"
                "ds_read_b32 %6, %32 offset:24\n"
                "ds_read_b32 %7, %32 offset:28\n"
                "ds_read_b32 %8, %32 offset:32\n"
                "ds_read_b32 %9, %32 offset:36\n"
                "ds_read_b32 %10, %32 offset:40\n"
                "ds_read_b32 %11, %32 offset:44\n"
                "ds_read_b32 %12, %32 offset:48\n"
                "ds_read_b32 %13, %32 offset:52\n"
                "ds_read_b32 %14, %32 offset:56\n"
                "ds_read_b32 %15, %32 offset:60\n"
                "ds_read_b32 %16, %33 offset:0\n"
                "ds_read_b32 %17, %33 offset:4\n"
                "ds_read_b32 %18, %33 offset:8\n"
                "ds_read_b32 %19, %33 offset:12\n"
                "ds_read_b32 %20, %33 offset:16\n"
                "ds_read_b32 %21, %33 offset:20\n"
                "ds_read_b32 %22, %33 offset:24\n"
                "ds_read_b32 %23, %33 offset:28\n"
                "ds_read_b32 %24, %33 offset:32\n"
                "ds_read_b32 %25, %33 offset:36\n"
                "ds_read_b32 %26, %33 offset:40\n"
                "ds_read_b32 %27, %33 offset:44\n"
                "ds_read_b32 %28, %33 offset:48\n"
                "ds_read_b32 %29, %33 offset:52\n"
                "ds_read_b32 %30, %33 offset:56\n"
                "ds_read_b32 %31, %33 offset:60\n"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(av[0]), "=&v"(av[1]), "=&v"(av[2]), "=&v"(av[3]), "=&v"(av[4]), "=&v"(av[5]), "=&v"(av[6]), "=&v"(av[7]), "=&v"(av[8]), "=&v"(av[9]), "=&v"(av[10]), "=&v"(av[11]), "=&v"(av[12]), "=&v"(av[13]), "=&v"(av[14]), "=&v"(av[15]), "=&v"(rv[0]), "=&v"(rv[1]), "=&v"(rv[2]), "=&v"(rv[3]), "=&v"(rv[4]), "=&v"(rv[5]), "=&v"(rv[6]), "=&v"(rv[7]), "=&v"(rv[8]), "=&v"(rv[9]), "=&v"(rv[10]), "=&v"(rv[11]), "=&v"(rv[12]), "=&v"(rv[13]), "=&v"(rv[14]), "=&v"(rv[15])
            : "v"(pa), "v"(pr)
            : "memory");
    } else if constexpr (NR == 4) {
        asm volatile(
                "ds_read_b32 %0, %8 offset:0\n"
                "ds_read_b32 %1, %8 offset:4\n"
                "ds_read_b32 %2, %8 offset:8\n"
                "ds_read_b32 %3, %8 offset:12\n"
                "ds_read_b32 %4, %9 offset:0\n"
                "ds_read_b32 %5, %9 offset:4\n"
                "ds_read_b32 %6, %9 offset:8\n"
                "ds_read_b32 %7, %9 offset:12\n"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(av[0]), "=&v"(av[1]), "=&v"(av[2]), "=&v"(av[3]), "=&v"(rv[0]), "=&v"(rv[1]), "=&v"(rv[2]), "=&v"(rv[3])
            : "v"(pa), "v"(pr)
            : "memory");
    } else {
        asm volatile(
                "ds_read_b32 %0, %16 offset:0\n"
                "ds_read_b32 %1, %16 offset:4\n"
                "ds_read_b32 %2, %16 offset:8\n"
                "ds_read_b32 %3, %16 offset:12\n"
                "ds_read_b32 %4, %16 offset:16\n"
                "ds_read_b32 %5, %16 offset:20\n"
                "ds_read_b32 %6, %16 offset:24\n"
                "ds_read_b32 %7, %16 offset:28\n"
                "ds_read_b32 %8, %17 offset:0\n"
                "ds_read_b32 %9, %17 offset:4\n"
                "ds_read_b32 %10, %17 offset:8\n"
                "ds_read_b32 %11, %17 offset:12\n"
                "ds_read_b32 %12, %17 offset:16\n"
                "ds_read_b32 %13, %17 offset:20\n"
                "ds_read_b32 %14, %17 offset:24\n"
                "ds_read_b32 %15, %17 offset:28\n"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(av[0]), "=&v"(av[1]), "=&v"(av[2]), "=&v"(av[3]), "=&v"(av[4]), "=&v"(av[5]), "=&v"(av[6]), "=&v"(av[7]), "=&v"(rv[0]), "=&v"(rv[1]), "=&v"(rv[2]), "=&v"(rv[3]), "=&v"(rv[4]), "=&v"(rv[5]), "=&v"(rv[6]), "=&v"(rv[7])
            : "v"(pa), "v"(pr)
            : "memory");
    }
    // reads past this slice's end belong to the next slice (a split point
    // counted twice leaves the minimum unchanged): only the row end Tt masks
    const int lim = Tt - t0;
    if (__ballot(lim < NR - 1) == 0) {
#pragma unroll
        for (int k = 0; k < NR; k += 2) {
            sp0 = pmin(sp0, padd(rv[k], av[k]));
            sp1 = pmin(sp1, padd(rv[k + 1], av[k + 1]));
        }
    } else {
#pragma unroll
        for (int k = 0; k < NR; k += 2) {
            sp0 = pmin(sp0, padd(rv[k], k <= lim ? av[k] : INF16));
            sp1 = pmin(sp1, padd(rv[k + 1], k + 1 <= lim ? av[k + 1] : INF16));
        }
    }
}

// M: the split part of qm for span s (lanes = cells x
// slices of the split points, mfe_cells.hip): min over t >= 5 of
// qm(i, i+t-1) + qm1(i+t, j), written to the span's slot for F
__device__ __forceinline__ void split_rows(const CP &L, const Band &bd, int s, int lane) {
    const int N = bd.N, NP = L.np;
    if (s < 9 || s > N - 3) return;   // no split point below span 9
    __builtin_amdgcn_s_setprio(PRIO_ROLE);
    const int lo = bd.qlo(s), hi = bd.qhi(s);
    const int Lm = lanesets(hi - lo + 1);
    const int Tt = s - 4;
    u32 *slot = L.mla + (s % 6) * NP;
    for (int ls = 0; ls < Lm; ls++) {
        const int nc = min(WAVE, hi - lo + 1 - ls * WAVE);
        const int lc = nc <= 1 ? 0 : 32 - __clz(nc - 1);
        const int cst = 1 << lc, lsl = 6 - lc;
        const int c = lane & (cst - 1), rr = lane >> lc;
        int i = lo + ls * WAVE + c;
        const bool valid = c < nc;
        if (!valid) i = hi;
        const int j = i + s;
        const int nb = Tt - 4;                                  // split points t = 5..Tt
        const int bs = nb > 0 ? (nb + (1 << lsl) - 1) >> lsl : 0;
        u32 sp0 = INF16, sp1 = INF16;
        // split points in chunks of 16 and a last chunk of 16, 8 or 4 (bs is uniform;
        // round 5: +0.7 %, reads past a slice's end cost as much as the ones in it)
        int t0 = 5 + rr * bs;
        for (int ch = 0; ch < (bs >> 4); ch++, t0 += 16) split_chunk<16>(L, N, i, j, Tt, t0, sp0, sp1);
        const int rem = bs & 15;
        if (rem > 8) split_chunk<16>(L, N, i, j, Tt, t0, sp0, sp1);
        else if (rem > 4) split_chunk<8>(L, N, i, j, Tt, t0, sp0, sp1);
        else if (rem > 0) split_chunk<4>(L, N, i, j, Tt, t0, sp0, sp1);
        u32 split = pmin(sp0, sp1);
        for (int k = cst; k < WAVE; k <<= 1) split = pmin(split, u32(__shfl_xor(int(split), k, WAVE)));
        if (valid && rr == 0) slot[i] = pfin(split);
    }
    __builtin_amdgcn_s_setprio(0);
}

// Q: q5[j] for j = d-3, d-2 in one pass over k (qbm spans <= d-3 are final)
__device__ __forceinline__ void q5_columns(const CP &L, const Band &bd, int d, int lane) {
    const int N = bd.N, m_lo = bd.m_lo;
    const bool incr = bd.incr;
    const int j0 = d - 3, j1 = d - 2;
    const bool w0 = j0 >= 5 && j0 <= N && (!incr || j0 >= m_lo - 1);
    const bool w1 = j1 >= 5 && j1 <= N && (!incr || j1 >= m_lo - 1);
    if (w0 || w1) {
        __builtin_amdgcn_s_setprio(PRIO_ROLE);
        // the last step of an odd N has j1 = N + 1 (w1 false): its chain reads
        // column N instead, so no read leaves the tables (the result is unused)
        const int j1r = j1 <= N ? j1 : N;
        const int s0 = L.S[j0], s1 = L.S[j1r];
        const int sp0 = (j0 < N) ? L.S[j0 + 1] : 5, sp1 = (j1r < N) ? L.S[j1r + 1] : 5;   // no dangle past N
        u32 acc0 = INF16, acc1 = INF16;
        for (int k0 = 1; k0 <= j1r - 4; k0 += WAVE) {
            const int kk = k0 + lane;
            const bool ok1 = kk <= j1r - 4, ok0 = kk <= j0 - 4;
            const int k = ok1 ? kk : 1;
            const int sk = L.S[k], skm = (k > 1) ? L.S[k - 1] : 5;
            const u32 q5k = L.q5[k - 1];
            const int ix1 = off(j1r - k, N) + k - 1;
            const int ix0 = off(max(j0 - k, 4), N) + k - 1;
            const u32 ex1 = L.dt[DT_EXT + ptype(sk, s1) * 36 + skm * 6 + sp1];
            const u32 ex0 = L.dt[DT_EXT + ptype(sk, s0) * 36 + skm * 6 + sp0];
            const u32 t1 = padd(padd(q5k, L.qbm[ix1]), padd(L.ct[CT_INVMM + L.cc[ix1]], ex1));
            const u32 t0 = padd(padd(q5k, L.qbm[ix0]), padd(L.ct[CT_INVMM + L.cc[ix0]], ex0));
            acc1 = pmin(acc1, ok1 ? t1 : INF16);
            acc0 = pmin(acc0, ok0 ? t0 : INF16);
        }
        const u32 red0 = wave_min(acc0), red1 = wave_min(acc1);
        if (lane == 0) {
            u32 q0 = L.q5[j0];   // restored (refold) or initial when not recomputed
            if (w0) {
                q0 = pfin(pmin((L.up[j0] >= 1) ? L.q5[j0 - 1] : INF16, red0));
                L.q5[j0] = q0;
            }
            if (w1) L.q5[j1] = pfin(pmin((L.up[j1] >= 1) ? q0 : INF16, red1));
        }
        __builtin_amdgcn_s_setprio(0);
    }
}

// One instance per wave (WID): every wave's sweep holds only its own interior-loop
// block and roles, so the registers of the other waves' roles are not live in it
template <int NT, int NM, int WID>
__device__ __forceinline__ void mfe_pair_fold(const KArgs &ka, const DevScaled *__restrict__ XS,
                                              const DevTables *__restrict__ TT, const int *vs, const CP &L,
                                              const IncM &inc, const bool constrained, const int lane,
                                              const unsigned long long *sst) {
    const int N = uni(gld(&ka.variants[vs[0]].N));
    constexpr int wid = WID;
    constexpr int fls = FW[0] == wid ? 0 : (FW[1] == wid ? 1 : -1);   // this wave's finalize lane-set
    const u32 *gct = reinterpret_cast<const u32 *>(XS->ctab);
    const Band bd = inc.band(N);
    // (uni(): vector loads inside the kernel's loop, scalar registers through the sweep)
    const u32 mlclosing = u32(uni(int(__float_as_uint(gld(&XS->mlclosing)))));
    const u32 mlbase = u32(uni(int(__float_as_uint(gld(&XS->mlbase_sig)))));
    const u32 tauE = u32(uni(int(gld(gct + CT_FSM + 6))));
    const u32 fsm5 = u32(uni(int(gld(gct + CT_FSM + 5))));
    BUni U = buni(L, XS, N);
    U.fs1 = u32(uni(int(U.fs1)));
    if (wid == L_WAVE) {   // steps 0 (no B work: d + 1 < 8) and 1
        if (lane == 0) L.cnt[0] = 0;
        build_list(L, bd, lane, 8, 1);
    }
    __syncthreads();
    int cPP = 0;                // this step's list counts and first B record (load_list)
    u32 cwd = 0, cmm = 0;

#ifdef ADX_STAMP
    unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long st_sw0 = __builtin_amdgcn_s_memtime();
    unsigned long long st_last = st_sw0;
#ifndef ADX_STAMP_F
    st_acc[11] = sst[1];
    st_acc[12] = sst[2];
    st_acc[13] = sst[3];
#endif
    st_acc[7] = sst[4];
    st_acc[14] = sst[5];
    st_acc[15] = sst[6];
    st_acc[8] = sst[0] + (st_last - st_sw0);   // setup + the sweep's prelude
#endif
    // a fold from scratch is a refold whose hull clamps nowhere
    const int mloF = bd.incr ? bd.m_lo : -4096, mhiF = bd.incr ? bd.m_hi : 4096;
    FRun f{};
    // (the finalize wave holding PRIO_ROLE through its whole sweep instead of around F
    // measured -1.1 %: its loop top then takes issue slots from the block waves, which
    // set the step once F is this short; profiles/fanchor_ab.txt)
    int sl = 0;   // list slot of this step: step index % 3
    for (int d = 6; d - 3 <= N; d += 2) {
#ifdef ADX_STAMP
        if (N - (d - 2) <= 64 && N - (d - 4) > 64 && lane == 0 && wid < 16)   // the first late step
            for (int k = 0; k < 16; k++) atomicAdd(&g_stamps_pe[wid][k], st_acc[k]);
#endif
        const int sl1 = sl == 2 ? 0 : sl + 1, sl2 = sl1 == 2 ? 0 : sl1 + 1;
        PSTAMP(0);
        int nPP = 0;
        u32 nwd = 0, nmm = 0;
        if (wid < MFE_NBLK) load_list(L, lane, sl1, nPP, nwd, nmm);   // the next step's, built a step ago
        if (wid == L_WAVE) {   // L: diagonals d+4, d+5 (B's lanes two steps on; their qbm marks are the setup's)
            __builtin_amdgcn_s_setprio(PRIO_ROLE);
            build_list(L, bd, lane, d + 4, sl2);
            __builtin_amdgcn_s_setprio(0);
        }
        PSTAMP(1);
        if constexpr (fls >= 0) finalize<NM, fls>(L, f, U, N, d, lane, mloF, mhiF, mlclosing, mlbase PSTAMP_ARGS);
        PSTAMP(2);
        block_partials<wid>(L, ka.loop16, U, d, lane, sl, cPP, cwd, cmm, constrained, tauE, fsm5 PSTAMP_ARGS);
        cPP = nPP, cwd = nwd, cmm = nmm;
        PSTAMP(3);
        if (wid == MW[0] || wid == MW[1]) split_rows(L, bd, wid == MW[0] ? d : d + 1, lane);
        PSTAMP(4);
        if (wid == Q_WAVE) q5_columns(L, bd, d, lane);
        PSTAMP(5);
        lds_barrier();
        PSTAMP(6);
        sl = sl1;
    }
#ifdef ADX_STAMP
    if (lane == 0 && wid < 16)
        for (int k = 0; k < 16; k++) atomicAdd(&g_stamps_p[wid][k], st_acc[k]);
#endif
}

// the fold instance of wave w (one per wave: mfe_pair_fold's WID)
template <int NT, int NM, int... Ws>
__device__ __forceinline__ void pair_fold_wave(std::integer_sequence<int, Ws...>, int w, const KArgs &ka,
                                               const DevScaled *__restrict__ XS, const DevTables *__restrict__ TT,
                                               const int *vs, const CP &L, const IncM &inc, bool constrained,
                                               int lane, const unsigned long long *sst) {
    ((w == Ws ? (mfe_pair_fold<NT, NM, Ws>(ka, XS, TT, vs, L, inc, constrained, lane, sst), 0) : 0), ...);
}

// mfe_pair_kernel's arguments, one struct at the start of the argument segment
struct PairArgs {
    KArgs ka;
    const DevScaled *XS;
    const DevTables *TT;
    const uint8_t *seqs;   // [W][ka.Nraw]
    int W;
    float *gout;           // [W][ka.n_variants]
    const int *mask;       // 1 = fold (null: every walker)
};
static_assert(sizeof(PairArgs) % 4 == 0, "whole words");
struct ArgWords {
    uint32_t w[sizeof(PairArgs) / 4];
};

template <int NT, int NM>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(MFE_WPE, MFE_WPE)))
mfe_pair_kernel(const PairArgs args) {
    // Persistent workgroups over a queue of (walker, fold group) items in launch
    // order: item it is group it % ng of the walker at launch position it / ng
    // (ka.order: heaviest refolds first, the unscored walkers last and past the
    // bound).  Thread 0 takes the next index from the counter ka.pairq[0] and hands
    // it to the workgroup through the third word at PLay::FLAG.  No workgroup waits
    // for another, and every pass of the loop consumes one index of a counter that
    // only grows, so the loop ends after at most `items` passes whatever the number
    // of workgroups or their residency.  Every exit from the body is uniform (the
    // body has barriers): it and the walker's words are the same in every lane.
    //
    // The arguments are read again in every pass, through a pointer to the kernel's
    // argument segment that the compiler cannot see through: hoisted out of the loop,
    // the words a fold uses stay live across its whole sweep (measured at compile
    // time: 130 spilled SGPRs and 39 spilled VGPRs instead of 15 and none).
    // The thread's index goes the same way, or everything a fold derives from it
    // alone is computed once before the loop and kept in registers throughout.
    const CP L = PLay<NM>::carve();
    const int tid0 = threadIdx.x;
    const int ng = args.ka.n_groups2, W = args.W;
    const int items = (args.ka.order ? uni(min(max(args.ka.pairq[1], 0), W)) : W) * ng;
    int *const queue = args.ka.pairq;
    int nxt = 0;   // thread 0: the index of the item after this one, taken a whole fold ahead
    if (tid0 == 0) nxt = atomicAdd(queue, 1);
    pair_constants<NT, NM>(args.XS, args.TT, L);
    typedef __attribute__((address_space(4))) const PairArgs *kernarg_ptr;
    kernarg_ptr ap = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();   // `args` sits at its start
    for (;;) {
        int tid = tid0;
        asm volatile("" : "+s"(ap), "+v"(tid));
        ArgWords aw;   // (scalar loads; the words no pass uses are dropped)
#pragma unroll
        for (int k = 0; k < int(sizeof(PairArgs) / 4); k++) aw.w[k] = reinterpret_cast<const kc_u32 *>(ap)[k];
        const PairArgs A = __builtin_bit_cast(PairArgs, aw);
        const KArgs &ka = A.ka;
        const DevScaled *__restrict__ XS = A.XS;
        const DevTables *__restrict__ TT = A.TT;
        const uint8_t *seqs = A.seqs;
        float *gout = A.gout;
        const int *mask = A.mask;
        __syncthreads();   // the item before is done with the tables and the block_or words
        if (tid < 2) L.flag[tid] = 0;
        if (tid == 0) L.flag[2] = nxt;
        __syncthreads();
        const int it = uni(L.flag[2]);
        if (it >= items) break;
        if (tid == 0) nxt = atomicAdd(queue, 1);
        const int wb = it / ng, g = it - wb * ng;
        // (after the first pass's stores a load from global memory is a vector load
        // whatever its address: uni() puts what is uniform back into scalar registers)
        const WalkerRef wr = walker_ref(ka, mask, wb);
        if (!uni(int(wr.on))) continue;   // without an order list: a walker the mask leaves out
        const int w = uni(wr.w), cur = uni(wr.cur), c0 = uni(wr.c0), c1 = uni(wr.c1);
        const bool valid = uni(int(wr.valid)) != 0;
        const int vs[2] = {uni(gld(ka.groups2 + 2 * g)), uni(gld(ka.groups2 + 2 * g + 1))};
        // both in one word for the result (nothing in the sweep reads them; opaque, or the two
        // stay live through it as they are): the launcher bounds n_variants
        int vsp = vs[0] | (vs[1] << 16);
        asm volatile("" : "+s"(vsp));
        IncM inc{nullptr, nullptr, 0, 0, nullptr, nullptr};
        if (ka.tab) {
            inc = inc_slots(ka, w, g, cur);
            inc.dst = nullptr, inc.cc_dst = nullptr;   // (the write-back works them out)
            // a sibling group may clear tab_valid[w] on overflow while this one reads it:
            // either value is correct (an incremental refold equals a fold from scratch)
            if (valid && c0 >= 0) inc_refold(inc, ka, w, g, cur, c0, c1, uni(gld(&ka.variants[vs[0]].before_len)));
        }
        unsigned long long sst[7] = {0, 0, 0, 0, 0, 0, 0};
        // the folded length for the write-back, loaded here (one SGPR through the fold; the
        // address of the word, kept for a load after the sweep, was a spilled pair)
        const int N = uni(gld(&ka.variants[vs[0]].N));
        const bool constrained = pair_setup<NT, NM>(ka, XS, TT, vs, seqs + size_t(w) * ka.Nraw, L, inc, tid, sst);
        pair_fold_wave<NT, NM>(std::make_integer_sequence<int, NWV>{}, uni(tid / WAVE), ka, XS, TT, vs, L, inc,
                               constrained, tid & (WAVE - 1), sst);
        // the fold's write-back and 16-bit range check (one copy for all waves)
        const u32 z = L.q5[N];
        if (ka.tab) {
            // the slot the fold writes, worked out again from the walker's words (opaque, or the
            // addresses of the pass's start stay live through the sweep: two spilled pairs)
            int cw = cur;
            asm volatile("" : "+s"(cw));
            const IncM to = inc_slots(ka, w, g, cw);
            inc.dst = to.dst, inc.cc_dst = to.cc_dst;
        }
        const int ve[2] = {vsp & 0xFFFF, int(uint32_t(vsp) >> 16)};
        const bool bad = block_or(L.flag + 1, fold_writeback_once<NT>(ka, L, inc, N, tid));   // (mfe_cells.hip: __syncthreads_or)
        if (tid == 0) fold_result(ka, w, ve, gout, z, bad);
    }
}

template <int NM>
static hipError_t launch_pair_nm(const KArgs &ka, const uint8_t *seqs, int W, float *gout, const int *mask,
                                 hipStream_t stream, int grid) {
    constexpr size_t lds = PLay<NM>::BYTES;
    auto k = mfe_pair_kernel<NWV * WAVE, NM>;
    if (!ka.pairq || ka.n_variants > 0x10000) return hipErrorInvalidValue;   // (the kernel packs two variant indices in a word)
    // the carve addresses LDS from 0 (lds_at): no static LDS may precede the block
    hipError_t e = configure_dynamic_lds(k, lds, true);
    if (e != hipSuccess) return e;
    // the workgroups resident at once (asked once per instantiation): more would
    // only queue behind them for the same items
    static const int resident = [&]() {
        int nb = 0, dev = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void *>(k), NWV * WAVE, lds) !=
                hipSuccess ||
            hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return 0;
        return nb * cus;
    }();
    if (resident <= 0) return hipErrorLaunchFailure;
    const int items = W * ka.n_groups2;
    if (items <= 0) return hipSuccess;
    constexpr int GRID_MAX = 1 << 16;   // of ADX_PAIR_GRID: a workgroup past the items leaves at once
    const int wgs = grid > 0 ? std::min(grid, GRID_MAX) : std::min(items, resident);
    if (!ka.order) {   // with an order list order_kernel zeroed the counter
        e = hipMemsetAsync(ka.pairq, 0, sizeof(int), stream);
        if (e != hipSuccess) return e;
    }
    static bool reported = false;
    if (!reported && std::getenv("ADX_OCC")) {   // diagnostic: resident workgroups per CU at this LDS size
        hipFuncAttributes fa;
        int nb = 0;
        (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k));
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void *>(k), NWV * WAVE, lds);
        std::fprintf(stderr, "mfe_pair_kernel<%d>: %d waves, %zu B LDS, %d VGPRs, %d workgroups per CU\n", NM,
                     NWV, lds, fa.numRegs, nb);
    }
    reported = true;
    hipLaunchKernelGGL(k, dim3(wgs), dim3(NWV * WAVE), lds, stream, PairArgs{ka, ka.X, ka.T, seqs, W, gout, mask});
    return hipGetLastError();
}

}  // namespace

// The pair kernel covers folded lengths up to 100 (two 100-nt walkers per CU) and variant
// indices of 16 bits (it carries a group's two in one word).
bool mfe_pair_covers(const KArgs &ka) { return ka.Nmax <= 100 && ka.n_variants <= 0x10000; }

hipError_t launch_mfe_pair(const KArgs &ka, const uint8_t *seqs, int W, float *gout, const int *mask,
                           hipStream_t stream, int grid) {
    static_assert(PLay<100>::BYTES <= 80 * 1024, "two 100-nt walkers per CU");
    if (ka.Nmax <= 64) return launch_pair_nm<64>(ka, seqs, W, gout, mask, stream, grid);
    if (ka.Nmax <= 100) return launch_pair_nm<100>(ka, seqs, W, gout, mask, stream, grid);
    return hipErrorInvalidValue;
}

}  // namespace adx

#ifdef ADX_STAMP
extern "C" int adx_debug_stamps_pair(unsigned long long *out, int reset) {  // [16][16]
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(adx::g_stamps_p), sizeof(adx::g_stamps_p)) != hipSuccess) return 1;
    if (reset) {
        static unsigned long long z[16][16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(adx::g_stamps_p), z, sizeof(z)) != hipSuccess) return 2;
    }
    return 0;
}
extern "C" int adx_debug_stamps_pair_early(unsigned long long *out, int reset) {  // [16][16]: the early steps' share
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(adx::g_stamps_pe), sizeof(adx::g_stamps_pe)) != hipSuccess) return 1;
    if (reset) {
        static unsigned long long z[16][16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(adx::g_stamps_pe), z, sizeof(z)) != hipSuccess) return 2;
    }
    return 0;
}
#endif
