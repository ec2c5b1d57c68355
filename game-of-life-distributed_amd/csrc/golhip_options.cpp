// golhip_options.cpp — golhip_set_option and its neighbours: one table of
// the options, their accepted values and the consent each needs.
#include "golhip_impl.h"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>

namespace gh GOLHIP_HIDDEN {

// Options whose results are wrong by design (they isolate a cost) need the
// environment's explicit consent: GOLHIP_MEASUREMENT=1.
static bool measurement_env() {
    const char *v = getenv("GOLHIP_MEASUREMENT");
    return v && !strcmp(v, "1");
}
// Test hooks (exact results, but they force failure paths: a band that never
// publishes, a reported co-residency failure) need GOLHIP_TEST_HOOKS=1.
bool test_hooks_env() {
    const char *v = getenv("GOLHIP_TEST_HOOKS");
    return v && !strcmp(v, "1");
}
// Result-neutral A/B knobs of the kernel plans: the
// defaults are the plans the sweeps under profiles/ chose, and a product
// caller has no reason to move them, so they need GOLHIP_TUNING=1 (or the
// stronger GOLHIP_MEASUREMENT=1).
bool tuning_env() {
    const char *v = getenv("GOLHIP_TUNING");
    return (v && !strcmp(v, "1")) || measurement_env();
}

namespace {

// Who may set an option: anyone (product), or a caller whose environment
// consents to A/B tuning knobs, to wrong results, to test hooks (above).
// kPathSwitch: a tuning knob that only picks between two code paths of one
// plan (same launches, same results); it needs the tuning consent too, but
// golhip_build_info()'s CONSENT_TUNING names the knobs of the plans alone.
// kUnlisted: golhip_build_info()'s lists do not name the option (a hook that
// gives the same boards through another kernel, like kPathSwitch's knobs).
enum Consent : unsigned { kProduct = 1, kTuning = 2, kMeasurement = 4, kTestHook = 8, kPathSwitch = 16, kUnlisted = 32 };

constexpr int64_t kAny = INT64_MAX;  // lo = -kAny, hi = kAny: every value

struct Option {
    const char *key;
    unsigned consent;
    int64_t lo, hi;      // accepted range ...
    uint32_t members;    // ... of it only the values v with bit v set (0: all) ...
    bool or_zero;        // ... and 0 besides
    int golhip::*field;  // where the value goes (boolean: value != 0); null: the handler stores it
    bool boolean;
    bool clears_rpw;     // the automatic rows per wave depend on it: drop their cache
    int (*handler)(golhip_t h, int64_t value);  // after the range check, instead of the consent rule and the store
};

int set_trace(golhip_t h, int64_t value) {
    if (value && !h->d_trace) {
        if (hipMalloc(&h->d_trace, kTraceWords * sizeof(unsigned long long)) != hipSuccess)
            return fail(GOLHIP_ENOMEM, "trace buffer");
        if (hipMemsetAsync(h->d_trace, 0, kTraceWords * sizeof(unsigned long long), h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess)
            return fail(GOLHIP_EHIP, "trace buffer memset");
    }
    return GOLHIP_OK;
}

int set_timing(golhip_t h, int64_t value) {  // GOLHIP_FLAG_TIMING after creation (HIP events cost ~5 us a launch)
    if (value) h->flags |= GOLHIP_FLAG_TIMING;
    else h->flags &= ~GOLHIP_FLAG_TIMING;
    return GOLHIP_OK;
}

int set_cu_count(golhip_t h, int64_t value) {  // measurement: plan launches for fewer CUs (0: all of the device's)
    if (value < 0 || value > h->dev_cu) return fail(GOLHIP_EINVAL, "cu_count %lld not in 0..%d", (long long)value, h->dev_cu);
    h->cu_count = value ? (int)value : h->dev_cu;
    return GOLHIP_OK;
}

int set_persist_timeout_us(golhip_t h, int64_t value) {
    h->persist_timeout_ticks = value * 100;  // s_memrealtime: 100 MHz
    return GOLHIP_OK;
}

int set_flip_debug(golhip_t h, int64_t value) {
    // 1 no look-back, 2 no entries (measurement only: wrong lists); 4 report a
    // co-residency failure once (tests the ticket-order fallback; lists exact)
    if ((value & 3) && !measurement_env())
        return fail(GOLHIP_EINVAL, "flip_debug %lld gives wrong lists: measurement runs only (GOLHIP_MEASUREMENT=1)",
                    (long long)value);
    if ((value & 4) && !test_hooks_env()) return fail(GOLHIP_EINVAL, "flip_debug 4 is a test hook (GOLHIP_TEST_HOOKS=1)");
    h->flip_debug = (int)value;
    return GOLHIP_OK;
}

#define RANGE(lo, hi) lo, hi, 0, false
#define BOOLEAN -kAny, kAny, 0, false
constexpr uint32_t bits(std::initializer_list<int> vs) {
    uint32_t m = 0;
    for (int v : vs) m |= 1u << v;
    return m;
}

// Every option golhip_set_option knows.  The order within a consent class is
// the order golhip_build_info() lists it in (tests/test_abi_cpu.py pins it).
constexpr Option kOptions[] = {
    {"wpl", kProduct, 0, 4, bits({0, 1, 2, 4}), false, &golhip::wpl_opt, false, true, nullptr},
    {"persistent", kProduct, RANGE(-1, 1), &golhip::persistent, false, false, nullptr},
    {"lds_band", kProduct, RANGE(-1, 1), &golhip::lds_band, false, false, nullptr},
    {"skew", kProduct, RANGE(0, 2), &golhip::skew, false, false, nullptr},
    {"timing", kProduct, BOOLEAN, nullptr, true, false, set_timing},
    {"persist_timeout_us", kProduct, RANGE(1, 60000000), nullptr, false, false, set_persist_timeout_us},
    {"force_halo", kProduct, BOOLEAN, &golhip::force_halo, true, false, nullptr},
    {"persist_depth", kTuning, RANGE(0, GOLHIP_MAX_TB_DEPTH), &golhip::persist_depth, false, false, nullptr},
    {"persist_waves", kTuning, 0, 16, bits({0, 4, 8, 16}), false, &golhip::persist_waves, false, false, nullptr},
    {"dummy_rows", kTuning, RANGE(0, kHalo), &golhip::dummy_rows, false, false, nullptr},
    {"paired_bands", kTuning, RANGE(0, 1), &golhip::paired_bands, false, true, nullptr},
    {"persist_half", kTuning, RANGE(0, 1), &golhip::persist_half, false, false, nullptr},
    {"persist_wg_tx", kTuning, RANGE(0, 16), &golhip::persist_wg_tx, false, false, nullptr},
    {"trace", kTuning, BOOLEAN, nullptr, true, false, set_trace},
    {"cu_count", kTuning, BOOLEAN, nullptr, false, true, set_cu_count},  // (its bound is the device's: the handler checks)
    {"fill_skip", kTuning, BOOLEAN, &golhip::fill_skip, true, true, nullptr},
    {"skew_young", kTuning, 10, 400, 0, true, &golhip::skew_young, false, false, nullptr},
    {"skew_hcap", kTuning, RANGE(-1, 256), &golhip::skew_hcap, false, false, nullptr},
    {"skew_prio", kTuning, RANGE(0, 1), &golhip::skew_prio, false, false, nullptr},
    {"skew_half", kTuning, RANGE(-1, 1), &golhip::skew_half, false, false, nullptr},
    {"skew_tx", kTuning, RANGE(0, 2), &golhip::skew_tx, false, false, nullptr},
    {"lds_depth", kTuning, RANGE(0, 64), &golhip::lds_depth, false, false, nullptr},
    {"lds_waves", kTuning, 0, 16, bits({0, 8, 16}), false, &golhip::lds_waves, false, false, nullptr},
    {"lds_wg_cu", kTuning, RANGE(1, 2), &golhip::lds_wg_cu, false, false, nullptr},
    {"lds_age", kTuning, 25, 400, 0, true, &golhip::lds_age, false, false, nullptr},
    {"lds_pre", kTuning, RANGE(0, 64), &golhip::lds_pre, false, false, nullptr},
    {"lds_stride", kTuning, RANGE(0, 1), &golhip::lds_stride, false, false, nullptr},
    {"lds_xcd", kTuning, RANGE(0, 1), &golhip::lds_xcd, false, false, nullptr},
    {"flip_overlap", kTuning, RANGE(0, 3), &golhip::flip_overlap, false, false, nullptr},
    {"skew_pairs", kTuning, RANGE(0, 7), &golhip::skew_pairs, false, false, nullptr},
    // K1w's interior main-loop body (gol_skew_span.h); 0: an empty span, the general body alone
    {"skew_interior", kPathSwitch, RANGE(0, 1), &golhip::skew_interior, false, false, nullptr},
    // measurement only: the halo rows go stale (wrong results)
    {"halo_skip", kMeasurement, BOOLEAN, &golhip::halo_skip, true, false, nullptr},
    {"resident_fault", kTestHook, RANGE(0, 2), &golhip::resident_fault, false, false, nullptr},
    // test hook: several resident launches in one step
    {"resident_max_turns", kTestHook, RANGE(1, golk::kResidentMaxTurns), &golhip::resident_max, false, false, nullptr},
    {"flip_debug", kMeasurement | kTestHook, RANGE(0, 7), nullptr, false, false, set_flip_debug},  // (by bit: the handler)
    // test hook: 1 a Conway handle steps on K11 too (its static policy), 2 K11's dynamic policy for
    // every rule, the listed ones included; the reference's golden boards then judge both policies
    {"rule_kernel", kTestHook | kUnlisted, RANGE(0, 2), &golhip::rule_kernel, false, true, nullptr},
};
#undef RANGE
#undef BOOLEAN

const Option *find_option(const char *key) {
    for (const Option &o : kOptions)
        if (!strcmp(key, o.key)) return &o;
    return nullptr;
}

bool accepts(const Option &o, int64_t v) {
    if (o.or_zero && v == 0) return true;
    return v >= o.lo && v <= o.hi && (!o.members || (o.members >> v & 1));
}

// EINVAL with the key, the value and what the option accepts ("0 or 10..400", "{0,4,8,16}").
int refuse(const Option &o, int64_t value) {
    if (!o.members)
        return fail(GOLHIP_EINVAL, "%s %lld not in %s%lld..%lld", o.key, (long long)value, o.or_zero ? "0 or " : "",
                    (long long)o.lo, (long long)o.hi);
    char set[128] = "";
    for (int v = 0, n = 0; v < 32; ++v)
        if (o.members >> v & 1) n += snprintf(set + n, sizeof set - n, n ? ",%d" : "%d", v);
    return fail(GOLHIP_EINVAL, "%s %lld not in {%s}", o.key, (long long)value, set);
}

// The keys of one consent class, as golhip_build_info() lists them
// (flip_debug belongs to two classes by bit).
std::string consent_list(unsigned cls) {
    std::string s;
    for (const Option &o : kOptions) {
        if (!(o.consent & cls) || (o.consent & kUnlisted)) continue;
        if (!s.empty()) s += ",";
        s += o.key;
        if (o.handler == set_flip_debug) s += cls == kMeasurement ? ":1-3" : ":4";
    }
    return s;
}

}  // namespace
}  // namespace gh

using namespace gh;

extern "C" {

// The kernels' build macros, then the consent-gated options (the CPU suite
// checks the lists against the product contract).
const char *golhip_build_info(void) {
    static const std::string info = [] {
        std::string s = golk::build_info();
        s += " CONSENT_MEASUREMENT=" + consent_list(kMeasurement);
        s += " CONSENT_TEST_HOOKS=" + consent_list(kTestHook) + ",golhip_test_ring_init";
        s += " CONSENT_TUNING=" + consent_list(kTuning);
        s += " PRODUCT_OPTIONS=" + consent_list(kProduct);
        return s;
    }();
    return info.c_str();
}

int golhip_set_tb_depth(golhip_t h, int32_t t) {
    if (int rc = check(h)) return rc;
    if (t < 1 || t > GOLHIP_MAX_TB_DEPTH) return fail(GOLHIP_EINVAL, "tb depth %d not in 1..%d", t, GOLHIP_MAX_TB_DEPTH);
    std::lock_guard<std::mutex> g(h->mu);
    h->tb_depth = t;
    return GOLHIP_OK;
}

int golhip_set_rows_per_wave(golhip_t h, int32_t r) {
    if (int rc = check(h)) return rc;
    if (r < 0) return fail(GOLHIP_EINVAL, "rows per wave %d", r);
    std::lock_guard<std::mutex> g(h->mu);
    h->rows_per_wave = r;
    return GOLHIP_OK;
}

// The checks in order: key, tuning consent, (lock,) accepted values, then
// measurement / test-hook consent for a value other than 0.
int golhip_set_option(golhip_t h, const char *key, int64_t value) {
    if (int rc = check(h)) return rc;
    if (!key) return fail(GOLHIP_EINVAL, "null option");
    const Option *o = find_option(key);
    if (o && (o->consent & (kTuning | kPathSwitch)) && !tuning_env())
        return fail(GOLHIP_EINVAL, "%s is an A/B tuning knob of the kernel plans: set GOLHIP_TUNING=1", key);
    std::lock_guard<std::mutex> g(h->mu);
    if (!o) return fail(GOLHIP_EINVAL, "unknown option %s", key);
    if (!accepts(*o, value)) return refuse(*o, value);
    if (o->handler) {
        if (int rc = o->handler(h, value)) return rc;
    } else {
        if (value && (o->consent & kMeasurement) && !measurement_env())
            return fail(GOLHIP_EINVAL, "%s gives wrong results: measurement runs only (GOLHIP_MEASUREMENT=1)", key);
        if (value && (o->consent & kTestHook) && !test_hooks_env())
            return fail(GOLHIP_EINVAL, "%s is a test hook (GOLHIP_TEST_HOOKS=1)", key);
        h->*(o->field) = o->boolean ? value != 0 : (int)value;
    }
    if (o->clears_rpw)
        for (int &c : h->auto_rpw) c = 0;
    return GOLHIP_OK;
}

}  // extern "C"
