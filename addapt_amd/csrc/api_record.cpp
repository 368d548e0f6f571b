// C ABI of the MI355X engine (include/addapt_gpu.h), what reads a context's
// record of its steps: picks, autocorrelation and designs, each with its
// stateless form on caller-supplied trajectories.
#include <cctype>

#include "api_ctx.hpp"
#include "traj_autocorr_core.hpp"

using namespace adx;

// ================================================================== picks
// (traj_pick.hip; the rule: traj_pick_core.hpp)
namespace {

adx_status pick_args_ok(const char *who, int S, int window, int cap) {
    if (window < 1)
        return fail(ADX_EINVAL, "%s: window %d < 1 (cap must be at least ceil(steps / window))", who, window);
    const int need = (S - 1) / window + 1;
    if (cap < need)
        return fail(ADX_EINVAL, "%s: cap %d too small: %d steps with window %d need cap >= %d", who, cap, S, window,
                    need);
    return ADX_OK;
}

// picks of W step-major device trajectories, chunk by chunk (keys / bad: scratch the caller frees)
adx_status pick_device(const double *dscores, int W, int S, int window, int cap, DevBuf<uint64_t> &keys,
                       DevBuf<int> &bad, int *dn, int32_t *dsteps, double *dpick, hipStream_t stream) {
    const int chunk = traj_pick_chunk(S, W);
    MEM_TRY(keys.alloc(traj_pick_key_words(S, chunk)));
    MEM_TRY(bad.alloc(size_t(chunk)));
    for (int w0 = 0; w0 < W; w0 += chunk)
        HIP_TRY(launch_traj_pick(dscores, W, S, window, cap, w0, std::min(chunk, W - w0), keys.p, bad.p, dn, dsteps,
                                 dpick, stream));
    return ADX_OK;
}

}  // namespace

extern "C" adx_status adx_pick_scores(int device, int n_traj, int n_steps, const double *scores, int window, int cap,
                                      int *n_picks, int32_t *steps) {
    if (n_traj < 1 || n_steps < 1 || n_steps > PICK_MAX_STEPS || !scores || !n_picks || !steps)
        return fail(ADX_EINVAL, "adx_pick_scores: bad argument");
    adx_status s = pick_args_ok("adx_pick_scores", n_steps, window, cap);
    if (s) return s;
    DeviceStream dev;
    s = dev.open(device);
    if (s) return s;
    const size_t R = size_t(n_steps) * size_t(n_traj), O = size_t(n_traj) * size_t(cap);
    DevBuf<double> dsc;
    DevBuf<int> dn, bad;
    DevBuf<int32_t> dst;
    DevBuf<uint64_t> keys;
    MEM_TRY(dsc.alloc(R));
    MEM_TRY(dn.alloc(size_t(n_traj)));
    MEM_TRY(dst.alloc(O));
    HIP_TRY(hipMemcpyAsync(dsc.p, scores, R * sizeof(double), hipMemcpyHostToDevice, dev.stream));
    HIP_TRY(hipMemsetAsync(dst.p, 0xff, O * sizeof(int32_t), dev.stream));
    s = pick_device(dsc.p, n_traj, n_steps, window, cap, keys, bad, dn.p, dst.p, nullptr, dev.stream);
    if (s) return s;
    HIP_TRY(hipMemcpyAsync(n_picks, dn.p, sizeof(int) * size_t(n_traj), hipMemcpyDeviceToHost, dev.stream));
    HIP_TRY(hipMemcpyAsync(steps, dst.p, O * sizeof(int32_t), hipMemcpyDeviceToHost, dev.stream));
    HIP_TRY(hipStreamSynchronize(dev.stream));
    return ADX_OK;
}

extern "C" adx_status adx_record_begin(adx_ctx *c, int max_steps) {
    if (!c || max_steps < 1 || max_steps > PICK_MAX_STEPS) return fail(ADX_EINVAL, "adx_record_begin: bad argument");
    if (c->W <= 0) return fail(ADX_ESTATE, "adx_record_begin before adx_walkers_init");
    auto &rec = c->rec;
    rec.clear();
    const size_t W = size_t(c->W), N = size_t(c->pb.Nraw), R = size_t(max_steps) * W;
    std::vector<int> posmap(N, -1);
    for (size_t m = 0; m < c->mut.size(); m++) posmap[size_t(c->mut[m])] = int(m);
    std::vector<uint8_t> lower(N);
    for (size_t k = 0; k < N; k++) lower[k] = std::islower(static_cast<unsigned char>(c->templ[k])) ? 1 : 0;
    hipError_t e = rec.cur.alloc(R);
    if (e == hipSuccess) e = rec.pos.alloc(R);
    if (e == hipSuccess) e = rec.out.alloc(R);
    if (e == hipSuccess) e = rec.base.alloc(R);
    if (e == hipSuccess) e = rec.seq0.alloc(W * N);
    if (e == hipSuccess) e = rec.posmap.upload(posmap.data(), N, c->pb.stream);
    if (e == hipSuccess) e = rec.lower.upload(lower.data(), N, c->pb.stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(rec.seq0.p, c->cur_seq.p, W * N, hipMemcpyDeviceToDevice, c->pb.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->pb.stream);   // posmap / lower are this call's locals
    if (e != hipSuccess) {
        rec.clear();
        (void)hipGetLastError();
        if (e == hipErrorOutOfMemory)
            return fail(ADX_ENOMEM, "adx_record_begin: %d steps x %zu walkers x 17 bytes do not fit the device",
                        max_steps, W);
        return fail(ADX_EHIP, "adx_record_begin: %s", hipGetErrorString(e));
    }
    rec.on = true;
    rec.max_steps = max_steps;
    rec.W = c->W;
    rec.step0 = c->step;
    return ADX_OK;
}

extern "C" adx_status adx_record_end(adx_ctx *c) {
    if (!c) return fail(ADX_EINVAL, "adx_record_end: null context");
    HIP_TRY(hipStreamSynchronize(c->pb.stream));
    c->rec.clear();
    return ADX_OK;
}

// what every call that reads the record requires: its arguments, a live record, a step in it
static adx_status record_ready(const adx_ctx *c, const char *who, bool args) {
    if (!c || !args) return fail(ADX_EINVAL, "%s: null argument", who);
    if (!c->rec.on) return fail(ADX_ESTATE, "%s before adx_record_begin", who);
    if (c->rec.broken)
        return fail(ADX_ESTATE, "%s: the record is broken (walkers initialised or imported during it, or "
                                "a failed adx_run_steps); begin a new one", who);
    if (c->rec.rows <= 0) return fail(ADX_ESTATE, "%s: no step recorded yet", who);
    return ADX_OK;
}

// a record's picks on the device: per walker their number and cap rows (-1 past the picks), scores, sequences
struct RecordPicks {
    DevBuf<int> dn, bad;
    DevBuf<int32_t> dst;
    DevBuf<double> dps;
    DevBuf<char> dseq;
    DevBuf<uint64_t> keys;
};

// Pick from the context's record and replay the picked steps into the sequences (with_seqs)
// and the caller's base counts (dcnt); neither: no replay.  ev: recorded before, between, after.
static adx_status record_picks_device(const adx_ctx *c, int window, int cap, bool with_seqs, unsigned long long *dcnt,
                                      RecordPicks &p, const Events *ev) {
    const auto &rec = c->rec;
    const hipStream_t stream = c->pb.stream;
    const int W = rec.W, N = c->pb.Nraw;
    const size_t O = size_t(W) * size_t(cap);
    MEM_TRY(p.dn.alloc(size_t(W)));
    MEM_TRY(p.dst.alloc(O));
    MEM_TRY(p.dps.alloc(O));
    HIP_TRY(hipMemsetAsync(p.dst.p, 0xff, O * sizeof(int32_t), stream));
    HIP_TRY(hipMemsetAsync(p.dps.p, 0, O * sizeof(double), stream));
    if (with_seqs) {
        MEM_TRY(p.dseq.alloc(O * size_t(N)));
        HIP_TRY(hipMemsetAsync(p.dseq.p, 0, O * size_t(N), stream));
    }
    if (ev) HIP_TRY(hipEventRecord((*ev)[0], stream));
    adx_status s = pick_device(rec.cur.p, W, rec.rows, window, cap, p.keys, p.bad, p.dn.p, p.dst.p, p.dps.p, stream);
    if (s) return s;
    if (ev) HIP_TRY(hipEventRecord((*ev)[1], stream));
    if (with_seqs || dcnt) {
        ReplayArgs a{};
        a.seq0 = rec.seq0.p;
        a.pos = rec.pos.p;
        a.base = rec.base.p;
        a.outcome = rec.out.p;
        a.W = W;
        a.N = N;
        a.rows = rec.rows;
        a.posmap = rec.posmap.p;
        a.clo_off = c->d_clo_off.p;
        a.clo_pos = c->d_clo_pos.p;
        a.clo_par = c->d_clo_par.p;
        a.lower = rec.lower.p;
        a.n_picks = p.dn.p;
        a.steps = p.dst.p;
        a.cap = cap;
        a.seqs = p.dseq.p;
        a.counts = dcnt;
        HIP_TRY(launch_traj_replay(a, stream));
    }
    if (ev) HIP_TRY(hipEventRecord((*ev)[2], stream));
    return ADX_OK;
}

extern "C" adx_status adx_record_picks(adx_ctx *c, int window, int cap, int *n_picks, int64_t *steps, double *scores,
                                       char *seqs, int64_t *base_counts) {
    adx_status s = record_ready(c, "adx_record_picks", n_picks && steps);
    if (s) return s;
    auto &rec = c->rec;
    Problem &pb = c->pb;
    const int W = rec.W, S = rec.rows, N = pb.Nraw;
    s = pick_args_ok("adx_record_picks", S, window, cap);
    if (s) return s;
    const size_t O = size_t(W) * size_t(cap);
    RecordPicks p;
    DevBuf<unsigned long long> dcnt;
    if (base_counts) {
        MEM_TRY(dcnt.alloc(size_t(N) * 4));
        HIP_TRY(hipMemsetAsync(dcnt.p, 0, size_t(N) * 4 * sizeof(unsigned long long), pb.stream));
    }
    Events ev;
    s = ev.create(3);
    if (!s) s = record_picks_device(c, window, cap, seqs != nullptr, dcnt.p, p, &ev);
    if (s) return s;
    std::vector<int32_t> rows(O);
    HIP_TRY(hipMemcpyAsync(n_picks, p.dn.p, sizeof(int) * size_t(W), hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipMemcpyAsync(rows.data(), p.dst.p, O * sizeof(int32_t), hipMemcpyDeviceToHost, pb.stream));
    if (scores) HIP_TRY(hipMemcpyAsync(scores, p.dps.p, O * sizeof(double), hipMemcpyDeviceToHost, pb.stream));
    if (seqs) HIP_TRY(hipMemcpyAsync(seqs, p.dseq.p, O * size_t(N), hipMemcpyDeviceToHost, pb.stream));
    if (base_counts)
        HIP_TRY(hipMemcpyAsync(base_counts, dcnt.p, size_t(N) * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    for (size_t k = 0; k < O; k++) steps[k] = rows[k] < 0 ? -1 : rec.step0 + rows[k];
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
    c->pick_ms = a;
    c->replay_ms = b;
    return ADX_OK;
}

extern "C" adx_status adx_last_pick_ms(const adx_ctx *c, double *pick_ms, double *replay_ms) {
    if (!c || !pick_ms || !replay_ms) return fail(ADX_EINVAL, "adx_last_pick_ms: null argument");
    *pick_ms = c->pick_ms;
    *replay_ms = c->replay_ms;
    return ADX_OK;
}

// ================================================================== autocorrelation
// (traj_autocorr.hip; the quantity and the correlation-time rule: traj_autocorr_core.hpp)
namespace {

adx_status autocorr_args_ok(const char *who, int rows, int max_lag, int discard) {
    if (discard < 0 || discard >= rows)
        return fail(ADX_EINVAL, "%s: discard %d outside 0..%d (%d steps)", who, discard, rows - 1, rows);
    const int kept = rows - discard;
    if (max_lag < 0 || max_lag > kept - 1)
        return fail(ADX_EINVAL, "%s: max_lag %d outside 0..%d: %d kept steps allow a lag of at most %d", who, max_lag,
                    kept - 1, kept, kept - 1);
    return ADX_OK;
}

}  // namespace

extern "C" adx_status adx_autocorr_codes(int device, int n_traj, int n_steps, int n_pos, const uint8_t *codes,
                                         int max_lag, int64_t *pos_matches, int64_t *traj_matches) {
    if (n_traj < 1 || n_steps < 1 || n_steps > PICK_MAX_STEPS || n_pos < 1 || !codes || !pos_matches)
        return fail(ADX_EINVAL, "adx_autocorr_codes: bad argument");
    adx_status s = autocorr_args_ok("adx_autocorr_codes", n_steps, max_lag, 0);
    if (s) return s;
    DeviceStream dev;
    s = dev.open(device);
    if (s) return s;
    const size_t L = size_t(max_lag) + 1, R = size_t(n_steps) * size_t(n_traj) * size_t(n_pos);
    DevBuf<uint8_t> dcodes;
    DevBuf<uint64_t> planes;
    DevBuf<unsigned long long> dpos, dtraj;
    DevBuf<int> bad;
    const int chunk = traj_autocorr_chunk(n_steps, n_pos, n_traj);
    MEM_TRY(dcodes.alloc(R));
    MEM_TRY(planes.alloc(traj_autocorr_plane_words(n_steps, n_pos, chunk)));
    MEM_TRY(dpos.alloc(size_t(n_pos) * L));
    MEM_TRY(bad.alloc(1));
    HIP_TRY(hipMemcpyAsync(dcodes.p, codes, R, hipMemcpyHostToDevice, dev.stream));
    HIP_TRY(hipMemsetAsync(dpos.p, 0, size_t(n_pos) * L * sizeof(unsigned long long), dev.stream));
    HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(int), dev.stream));
    if (traj_matches) {
        MEM_TRY(dtraj.alloc(size_t(n_traj) * L));
        HIP_TRY(hipMemsetAsync(dtraj.p, 0, size_t(n_traj) * L * sizeof(unsigned long long), dev.stream));
    }
    for (int w0 = 0; w0 < n_traj; w0 += chunk) {
        const int nw = std::min(chunk, n_traj - w0);
        HIP_TRY(launch_autocorr_pack_codes(dcodes.p, n_traj, n_steps, n_pos, w0, nw, planes.p, bad.p, dev.stream));
        HIP_TRY(launch_autocorr_lags(planes.p, nw, n_pos, n_steps, max_lag, w0, dpos.p, dtraj.p, dev.stream));
    }
    int wrong = 0;
    HIP_TRY(hipMemcpyAsync(&wrong, bad.p, sizeof(int), hipMemcpyDeviceToHost, dev.stream));
    HIP_TRY(hipMemcpyAsync(pos_matches, dpos.p, size_t(n_pos) * L * sizeof(int64_t), hipMemcpyDeviceToHost, dev.stream));
    if (traj_matches)
        HIP_TRY(hipMemcpyAsync(traj_matches, dtraj.p, size_t(n_traj) * L * sizeof(int64_t), hipMemcpyDeviceToHost,
                               dev.stream));
    HIP_TRY(hipStreamSynchronize(dev.stream));
    if (wrong) return fail(ADX_EINVAL, "adx_autocorr_codes: a code outside 1..4");
    return ADX_OK;
}

extern "C" adx_status adx_record_autocorr(adx_ctx *c, int max_lag, int discard, int64_t *pos_matches,
                                          int64_t *walker_matches, int64_t *base_counts, int64_t *outcome_counts,
                                          unsigned char *changeable, int *n_changeable) {
    adx_status s = record_ready(c, "adx_record_autocorr", pos_matches != nullptr);
    if (s) return s;
    auto &rec = c->rec;
    Problem &pb = c->pb;
    const int W = rec.W, S = rec.rows, N = pb.Nraw;
    s = autocorr_args_ok("adx_record_autocorr", S, max_lag, discard);
    if (s) return s;
    const int kept = S - discard;
    const size_t L = size_t(max_lag) + 1;
    // changeable: in the closure list of a freely mutable position (itself and its partners)
    std::vector<uint8_t> flag(size_t(N), 0);
    for (size_t m = 0; m + 1 < c->clo_off.size(); m++)
        for (int k = c->clo_off[m]; k < c->clo_off[m + 1]; k++) flag[size_t(c->clo_pos[size_t(k)])] = 1;
    std::vector<int> chg;
    for (int k = 0; k < N; k++)
        if (flag[size_t(k)]) chg.push_back(k);
    const int P = int(chg.size());
    for (int k = 0; k < N; k++)
        for (size_t l = 0; l < L; l++) pos_matches[size_t(k) * L + l] = int64_t(W) * int64_t(kept - int(l));
    if (walker_matches) std::fill(walker_matches, walker_matches + size_t(W) * L, int64_t(0));
    if (changeable) std::copy(flag.begin(), flag.end(), changeable);
    if (n_changeable) *n_changeable = P;
    DevBuf<int> dchg;
    DevBuf<uint8_t> dflag;
    DevBuf<uint64_t> planes;
    DevBuf<unsigned long long> dpos, dwalk, dbase, dout;
    const int chunk = traj_autocorr_chunk(kept, P, W);
    HIP_TRY(dchg.upload(chg.data(), chg.size(), pb.stream));
    HIP_TRY(dflag.upload(flag.data(), flag.size(), pb.stream));
    MEM_TRY(planes.alloc(traj_autocorr_plane_words(kept, P, chunk)));
    MEM_TRY(dpos.alloc(size_t(P) * L));
    MEM_TRY(dwalk.alloc(size_t(W) * L));
    MEM_TRY(dbase.alloc(size_t(N) * 4));
    MEM_TRY(dout.alloc(size_t(W) * 4));
    HIP_TRY(hipMemsetAsync(dpos.p, 0, std::max<size_t>(size_t(P) * L, 1) * sizeof(unsigned long long), pb.stream));
    HIP_TRY(hipMemsetAsync(dwalk.p, 0, size_t(W) * L * sizeof(unsigned long long), pb.stream));
    HIP_TRY(hipMemsetAsync(dbase.p, 0, size_t(N) * 4 * sizeof(unsigned long long), pb.stream));
    AutocorrPackArgs a{};
    a.seq0 = rec.seq0.p;
    a.pos = rec.pos.p;
    a.base = rec.base.p;
    a.outcome = rec.out.p;
    a.W = W;
    a.N = N;
    a.rows = S;
    a.discard = discard;
    a.posmap = rec.posmap.p;
    a.clo_off = c->d_clo_off.p;
    a.clo_pos = c->d_clo_pos.p;
    a.clo_par = c->d_clo_par.p;
    a.chg = dchg.p;
    a.changeable = dflag.p;
    a.P = P;
    a.nwords = ta_words(kept);
    a.planes = reinterpret_cast<unsigned long long *>(planes.p);
    a.base_counts = dbase.p;
    a.outcome_counts = dout.p;
    // pack and lag times summed over the chunks: an event before and after each launch
    const int n_chunks = (W + chunk - 1) / chunk;
    Events ev;
    s = ev.create(size_t(n_chunks) * 3);
    if (s) return s;
    for (int w0 = 0, i = 0; w0 < W; w0 += chunk, i++) {
        a.w0 = w0;
        a.nw = std::min(chunk, W - w0);
        HIP_TRY(hipEventRecord(ev[size_t(3 * i)], pb.stream));
        HIP_TRY(launch_autocorr_pack(a, pb.stream));
        HIP_TRY(hipEventRecord(ev[size_t(3 * i + 1)], pb.stream));
        HIP_TRY(launch_autocorr_lags(planes.p, a.nw, P, kept, max_lag, w0, dpos.p, dwalk.p, pb.stream));
        HIP_TRY(hipEventRecord(ev[size_t(3 * i + 2)], pb.stream));
    }
    std::vector<int64_t> hpos(std::max<size_t>(size_t(P) * L, 1));
    HIP_TRY(hipMemcpyAsync(hpos.data(), dpos.p, size_t(P) * L * sizeof(int64_t), hipMemcpyDeviceToHost, pb.stream));
    if (walker_matches)
        HIP_TRY(hipMemcpyAsync(walker_matches, dwalk.p, size_t(W) * L * sizeof(int64_t), hipMemcpyDeviceToHost,
                               pb.stream));
    if (base_counts)
        HIP_TRY(hipMemcpyAsync(base_counts, dbase.p, size_t(N) * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, pb.stream));
    if (outcome_counts)
        HIP_TRY(hipMemcpyAsync(outcome_counts, dout.p, size_t(W) * 4 * sizeof(int64_t), hipMemcpyDeviceToHost,
                               pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    for (int pi = 0; pi < P; pi++)
        std::copy(hpos.begin() + size_t(pi) * L, hpos.begin() + size_t(pi + 1) * L, pos_matches + size_t(chg[size_t(pi)]) * L);
    double pack = 0.0, lag = 0.0;
    for (int i = 0; i < n_chunks; i++) {
        float x = 0.f, y = 0.f;
        HIP_TRY(hipEventElapsedTime(&x, ev[size_t(3 * i)], ev[size_t(3 * i + 1)]));
        HIP_TRY(hipEventElapsedTime(&y, ev[size_t(3 * i + 1)], ev[size_t(3 * i + 2)]));
        pack += x;
        lag += y;
    }
    c->ac_pack_ms = pack;
    c->ac_lag_ms = lag;
    return ADX_OK;
}

extern "C" adx_status adx_last_autocorr_ms(const adx_ctx *c, double *pack_ms, double *lag_ms) {
    if (!c || !pack_ms || !lag_ms) return fail(ADX_EINVAL, "adx_last_autocorr_ms: null argument");
    *pack_ms = c->ac_pack_ms;
    *lag_ms = c->ac_lag_ms;
    return ADX_OK;
}

// ================================================================== designs
// (design_select.hip; the rule: design_select_core.hpp)
namespace {

// the device side of one selection over M entries: the buffers and their initial values
struct DesignWork {
    DevBuf<uint64_t> planes, rplanes, keys, keys_tmp, lead;
    DevBuf<int32_t> idx, idx_tmp, member_rank, leader_rank, member_of, sizes, leaders;
    DevBuf<int> hist, ctl;   // ctl: the kernels' flags [2] and state [3]
    DevBuf<unsigned long long> pair;
    DesignArgs a{};

    adx_status alloc(int M, int N, int radius, int K, bool with_hist, hipStream_t s) {
        const size_t m = size_t(M), pw = 2 * size_t((N + 63) / 64);
        MEM_TRY(planes.alloc(pw * m));
        MEM_TRY(rplanes.alloc(pw * m));
        MEM_TRY(keys.alloc(m));
        MEM_TRY(keys_tmp.alloc(m));
        MEM_TRY(idx.alloc(m));
        MEM_TRY(idx_tmp.alloc(m));
        MEM_TRY(hist.alloc(256 * size_t(design_sort_blocks(M))));
        MEM_TRY(ctl.alloc(5));
        MEM_TRY(member_rank.alloc(m));
        MEM_TRY(member_of.alloc(m));
        MEM_TRY(leader_rank.alloc(size_t(K)));
        MEM_TRY(lead.alloc(pw * size_t(K)));
        MEM_TRY(sizes.alloc(size_t(K)));
        MEM_TRY(leaders.alloc(size_t(K)));
        HIP_TRY(hipMemsetAsync(ctl.p, 0, 5 * sizeof(int), s));
        HIP_TRY(hipMemsetAsync(member_rank.p, 0xff, m * sizeof(int32_t), s));
        HIP_TRY(hipMemsetAsync(sizes.p, 0, size_t(K) * sizeof(int32_t), s));
        if (with_hist) {
            MEM_TRY(pair.alloc(size_t(N) + 1));
            HIP_TRY(hipMemsetAsync(pair.p, 0, (size_t(N) + 1) * sizeof(unsigned long long), s));
        }
        a.M = M;
        a.N = N;
        a.radius = radius;
        a.K = K;
        a.planes = planes.p;
        a.order = idx.p;
        a.rank_planes = rplanes.p;
        a.flags = ctl.p;
        a.state = ctl.p + 2;
        a.member_rank = member_rank.p;
        a.leader_rank = leader_rank.p;
        a.lead_planes = lead.p;
        a.member_of = member_of.p;
        a.sizes = sizes.p;
        a.leaders = leaders.p;
        return ADX_OK;
    }
};

adx_status design_args_ok(const char *who, int length, int radius, int max_designs) {
    if (length < 1 || length > 255)
        return fail(ADX_EINVAL, "%s: sequence length %d outside [1, 255]", who, length);
    if (radius < 0) return fail(ADX_EINVAL, "%s: radius %d < 0", who, radius);
    if (max_designs < 1) return fail(ADX_EINVAL, "%s: max_designs %d < 1", who, max_designs);
    return ADX_OK;
}

}  // namespace

extern "C" adx_status adx_select_designs(int device, int n_seqs, int length, const char *seqs, const double *scores,
                                         int radius, int max_designs, int *n_designs, int32_t *leaders, int32_t *sizes,
                                         int32_t *member_of, int64_t *pair_hist) {
    if (n_seqs < 1 || !seqs || !scores || !n_designs || !leaders || !sizes)
        return fail(ADX_EINVAL, "adx_select_designs: bad argument");
    adx_status s = design_args_ok("adx_select_designs", length, radius, max_designs);
    if (s) return s;
    DeviceStream dev;
    s = dev.open(device);
    if (s) return s;
    const int M = n_seqs, N = length, K = std::min(max_designs, M);
    DevBuf<char> dseq;
    DevBuf<double> dsc;
    DesignWork w;
    MEM_TRY(dseq.alloc(size_t(M) * N));
    MEM_TRY(dsc.alloc(size_t(M)));
    HIP_TRY(hipMemcpyAsync(dseq.p, seqs, size_t(M) * N, hipMemcpyHostToDevice, dev.stream));
    HIP_TRY(hipMemcpyAsync(dsc.p, scores, size_t(M) * sizeof(double), hipMemcpyHostToDevice, dev.stream));
    s = w.alloc(M, N, radius, K, pair_hist != nullptr, dev.stream);
    if (s) return s;
    HIP_TRY(launch_design_pack(dseq.p, dsc.p, N, M, nullptr, nullptr, 0, M, w.planes.p, w.keys.p, w.idx.p, nullptr,
                               w.a.flags, dev.stream));
    HIP_TRY(launch_design_order(w.keys.p, w.idx.p, w.keys_tmp.p, w.idx_tmp.p, M, w.hist.p, dev.stream));
    HIP_TRY(launch_design_select(w.a, dev.stream));
    if (pair_hist) HIP_TRY(launch_design_hist(w.a, w.pair.p, dev.stream));
    int ctl[5];
    HIP_TRY(hipMemcpyAsync(ctl, w.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, dev.stream));
    HIP_TRY(hipStreamSynchronize(dev.stream));
    if (ctl[DESIGN_BAD]) return fail(ADX_EINVAL, "adx_select_designs: a character outside ACGU / acgu");
    const size_t nd = size_t(ctl[2]);
    HIP_TRY(hipMemcpyAsync(leaders, w.leaders.p, nd * sizeof(int32_t), hipMemcpyDeviceToHost, dev.stream));
    HIP_TRY(hipMemcpyAsync(sizes, w.sizes.p, nd * sizeof(int32_t), hipMemcpyDeviceToHost, dev.stream));
    if (member_of)
        HIP_TRY(hipMemcpyAsync(member_of, w.member_of.p, size_t(M) * sizeof(int32_t), hipMemcpyDeviceToHost, dev.stream));
    if (pair_hist)
        HIP_TRY(hipMemcpyAsync(pair_hist, w.pair.p, (size_t(N) + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, dev.stream));
    HIP_TRY(hipStreamSynchronize(dev.stream));
    *n_designs = int(nd);
    return ADX_OK;
}

extern "C" adx_status adx_record_designs(adx_ctx *c, int window, int radius, int max_designs, int *n_designs,
                                         int32_t *walkers, int64_t *steps, double *scores, char *seqs, int32_t *sizes,
                                         int32_t *n_walkers, int64_t *n_picks_total, int64_t *pair_hist) {
    adx_status s = record_ready(c, "adx_record_designs", n_designs != nullptr);
    if (s) return s;
    auto &rec = c->rec;
    Problem &pb = c->pb;
    const int W = rec.W, S = rec.rows, N = pb.Nraw;
    if (window < 1) return fail(ADX_EINVAL, "adx_record_designs: window %d < 1", window);
    s = design_args_ok("adx_record_designs", N, radius, max_designs);
    if (s) return s;
    const int cap = (S - 1) / window + 1;
    const size_t O = size_t(W) * size_t(cap);
    if (O > size_t(0x7fffffff))
        return fail(ADX_EINVAL, "adx_record_designs: %d walkers x %d picks exceed 2^31 - 1 entries", W, cap);
    // the picks and their sequences, as adx_record_picks makes them, left on the device
    RecordPicks p;
    DevBuf<int> doff, dtotal;
    MEM_TRY(doff.alloc(size_t(W)));
    MEM_TRY(dtotal.alloc(1));
    s = record_picks_device(c, window, cap, true, nullptr, p, nullptr);
    if (s) return s;
    HIP_TRY(launch_design_offsets(p.dn.p, W, doff.p, dtotal.p, pb.stream));
    int M = 0;
    HIP_TRY(hipMemcpyAsync(&M, dtotal.p, sizeof(int), hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    p.keys.reset();
    if (n_picks_total) *n_picks_total = M;
    if (pair_hist) std::fill(pair_hist, pair_hist + N + 1, int64_t(0));
    *n_designs = 0;
    c->design_select_ms = c->design_hist_ms = 0.0;
    if (M == 0) return ADX_OK;   // no walker has a pick
    const int K = std::min(max_designs, M);
    DesignWork w;
    DevBuf<int32_t> src_of, dwalk, drow, dnw;
    DevBuf<double> dsc;
    DevBuf<char> dlead;
    s = w.alloc(M, N, radius, K, pair_hist != nullptr, pb.stream);
    if (s) return s;
    MEM_TRY(src_of.alloc(size_t(M)));
    MEM_TRY(dwalk.alloc(size_t(K)));
    MEM_TRY(drow.alloc(size_t(K)));
    MEM_TRY(dnw.alloc(size_t(K)));
    MEM_TRY(dsc.alloc(size_t(K)));
    MEM_TRY(dlead.alloc(size_t(K) * N));
    HIP_TRY(hipMemsetAsync(dnw.p, 0, size_t(K) * sizeof(int32_t), pb.stream));
    Events ev;
    s = ev.create(3);
    if (s) return s;
    HIP_TRY(hipEventRecord(ev[0], pb.stream));
    HIP_TRY(launch_design_pack(p.dseq.p, p.dps.p, N, int(O), p.dn.p, doff.p, cap, M, w.planes.p, w.keys.p, w.idx.p, src_of.p,
                               w.a.flags, pb.stream));
    HIP_TRY(launch_design_order(w.keys.p, w.idx.p, w.keys_tmp.p, w.idx_tmp.p, M, w.hist.p, pb.stream));
    HIP_TRY(launch_design_select(w.a, pb.stream));
    HIP_TRY(launch_design_walkers(w.a, src_of.p, cap, dnw.p, pb.stream));
    HIP_TRY(launch_design_gather(w.a, src_of.p, cap, p.dst.p, p.dps.p, p.dseq.p, dwalk.p, drow.p, dsc.p, dlead.p, pb.stream));
    HIP_TRY(hipEventRecord(ev[1], pb.stream));
    if (pair_hist) HIP_TRY(launch_design_hist(w.a, w.pair.p, pb.stream));
    HIP_TRY(hipEventRecord(ev[2], pb.stream));
    int ctl[5];
    HIP_TRY(hipMemcpyAsync(ctl, w.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    if (ctl[DESIGN_BAD]) return fail(ADX_EINVAL, "adx_record_designs: a recorded sequence holds a base outside ACGU");
    const size_t nd = size_t(ctl[2]);
    std::vector<int32_t> rows(nd);
    if (walkers) HIP_TRY(hipMemcpyAsync(walkers, dwalk.p, nd * sizeof(int32_t), hipMemcpyDeviceToHost, pb.stream));
    if (steps) HIP_TRY(hipMemcpyAsync(rows.data(), drow.p, nd * sizeof(int32_t), hipMemcpyDeviceToHost, pb.stream));
    if (scores) HIP_TRY(hipMemcpyAsync(scores, dsc.p, nd * sizeof(double), hipMemcpyDeviceToHost, pb.stream));
    if (seqs) HIP_TRY(hipMemcpyAsync(seqs, dlead.p, nd * size_t(N), hipMemcpyDeviceToHost, pb.stream));
    if (sizes) HIP_TRY(hipMemcpyAsync(sizes, w.sizes.p, nd * sizeof(int32_t), hipMemcpyDeviceToHost, pb.stream));
    if (n_walkers) HIP_TRY(hipMemcpyAsync(n_walkers, dnw.p, nd * sizeof(int32_t), hipMemcpyDeviceToHost, pb.stream));
    if (pair_hist)
        HIP_TRY(hipMemcpyAsync(pair_hist, w.pair.p, (size_t(N) + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, pb.stream));
    HIP_TRY(hipStreamSynchronize(pb.stream));
    if (steps)
        for (size_t d = 0; d < nd; d++) steps[d] = rec.step0 + rows[d];
    *n_designs = int(nd);
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
    c->design_select_ms = a;
    c->design_hist_ms = b;
    return ADX_OK;
}

extern "C" adx_status adx_last_design_ms(const adx_ctx *c, double *select_ms, double *hist_ms) {
    if (!c || !select_ms || !hist_ms) return fail(ADX_EINVAL, "adx_last_design_ms: null argument");
    *select_ms = c->design_select_ms;
    *hist_ms = c->design_hist_ms;
    return ADX_OK;
}
