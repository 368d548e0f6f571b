// The Monte Carlo context: api_ctx.cpp runs it, api_record.cpp reads its record
#pragma once

#include "api_problem.hpp"

struct adx_ctx {
    adx::Problem pb;
    std::string templ;
    std::vector<std::string> macrostates;
    std::vector<adx_term> terms;
    adx_thermostat thermo{};
    int n_contexts = 0;
    std::vector<int> mut;
    std::vector<int> clo_off, clo_pos, clo_err;
    std::vector<uint8_t> clo_par;
    std::vector<std::string> clo_msg;
    // walker state
    int W = 0;
    long long step = 0;
    adx::DevBuf<uint8_t> cur_seq;
    adx::DevBuf<double> cur_score, last_diff, auto_T, train;
    adx::DevBuf<uint32_t> mtA, mtC;
    adx::DevBuf<int64_t> counters;
    adx::DevBuf<int> ntrain, err;
    adx::DevBuf<uint8_t> prop_seq;
    adx::DevBuf<double> prop_score, temp, u;
    adx::DevBuf<int> changed, pick, bcode;
    adx::DevBuf<int> d_mut, d_clo_off, d_clo_pos, d_clo_err;
    adx::DevBuf<uint8_t> d_clo_par;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_ms = 0.0;
    std::string inside_kernel, outside_kernel;   // what the last adx_run_steps launched
    double score_ms_total = 0.0;   // sum of the score-kernel launch durations of the last run
    double inside_ms_total = 0.0, outside_ms_total = 0.0;   // the same windows split (inside, outside)
    int score_launches = 0;
    // The pick record (adx_record_begin): four of the trace's arrays kept on the
    // device for the whole run, [max_steps x W] step-major, the walkers' sequences
    // before its first step, and what the replay reads of the run-constant setup
    struct Record {
        bool on = false, broken = false;
        int max_steps = 0, rows = 0, W = 0;
        long long step0 = 0;   // the context's step index of row 0
        adx::DevBuf<double> cur;
        adx::DevBuf<int32_t> pos, out;
        adx::DevBuf<int8_t> base;
        adx::DevBuf<uint8_t> seq0, lower;
        adx::DevBuf<int> posmap;
        void clear() {
            on = broken = false;
            max_steps = rows = W = 0;
            cur.reset();
            pos.reset();
            out.reset();
            base.reset();
            seq0.reset();
            lower.reset();
            posmap.reset();
        }
        bool live() const { return on && !broken; }
    } rec;
    double pick_ms = 0.0, replay_ms = 0.0;   // the last adx_record_picks, from HIP events
    double ac_pack_ms = 0.0, ac_lag_ms = 0.0;   // the last adx_record_autocorr, from HIP events
    double design_select_ms = 0.0, design_hist_ms = 0.0;   // the last adx_record_designs, from HIP events

    ~adx_ctx() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};
