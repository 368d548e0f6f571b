// C ABI of the MI355X engine (include/addapt_gpu.h), the calls that need no
// device.  The device layers: api_fold.cpp (one fold), api_ctx.cpp (Monte Carlo
// contexts), api_record.cpp (picks, autocorrelation, designs).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <memory>

#include "api_common.hpp"
#include "traj_autocorr_core.hpp"

using namespace adx;

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;

adx_status adx::fail(adx_status s, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return s;
}

extern "C" const char *adx_last_error(void) { return g_err.c_str(); }
extern "C" int adx_abi_version(void) { return ADX_ABI_VERSION; }
extern "C" double adx_kT(void) { return kT_kcal(); }

// ------------------------------------------------------------------ params
extern "C" adx_status adx_params_load(const char *path, adx_params **out) {
    if (!path || !out) return fail(ADX_EINVAL, "adx_params_load: null argument");
    auto p = std::make_unique<adx_params>();
    std::string err;
    if (!load_params(path, p->P, err)) return fail(ADX_EPARAM, "%s", err.c_str());
    *out = p.release();
    return ADX_OK;
}

extern "C" void adx_params_free(adx_params *p) { delete p; }

extern "C" adx_status adx_eval_structure(const adx_params *p, const char *seq, const char *st,
                                         double *e) {
    if (!p || !seq || !st || !e) return fail(ADX_EINVAL, "adx_eval_structure: null argument");
    double v = eval_structure(p->P, seq, st);
    if (std::isnan(v)) return fail(ADX_EINVAL, "malformed structure '%s'", st);
    *e = v;
    return ADX_OK;
}

// ------------------------------------------------------------------ correlation time (traj_autocorr_core.hpp)
extern "C" adx_status adx_autocorr_time(const int64_t *matches, int max_lag, int64_t n_series, int64_t kept_steps,
                                        double baseline, int *tau) {
    if (!matches || !tau || max_lag < 0 || n_series < 1 || kept_steps < 1 || max_lag > kept_steps - 1)
        return fail(ADX_EINVAL, "adx_autocorr_time: bad argument (max_lag at most kept_steps - 1 = %lld)",
                    (long long)(kept_steps - 1));
    *tau = ta_time(matches, max_lag, n_series, kept_steps, baseline);
    return ADX_OK;
}
