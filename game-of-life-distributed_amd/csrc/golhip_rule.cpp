// golhip_rule.cpp — Life-like rules at the C-ABI: their spelling
// (gol_rule_text.h) and the rule of a handle.  What a rule changes in the
// plans is in golhip_plan.cpp and golhip_step.cpp (rule_path()).
#include "golhip_impl.h"
#include "gol_rule_text.h"

using namespace gh;

extern "C" {

int golhip_rule_parse(const char *text, uint32_t *birth, uint32_t *survive) {
    if (!text || !birth || !survive) return fail(GOLHIP_EINVAL, "null argument");
    std::string why;
    uint32_t b = 0, s = 0;
    if (!golrule::parse(text, &b, &s, &why)) return fail(GOLHIP_EINVAL, "%s", why.c_str());
    *birth = b;
    *survive = s;
    return GOLHIP_OK;
}

int golhip_rule_format(uint32_t birth, uint32_t survive, char *out, uint64_t cap) {
    if (!out) return fail(GOLHIP_EINVAL, "out is null");
    if (birth > golrule::kMaskAll || survive > golrule::kMaskAll)
        return fail(GOLHIP_EINVAL, "rule masks 0x%x / 0x%x above 0x1FF", birth, survive);
    const std::string s = golrule::format(birth, survive);
    if (s.size() + 1 > cap)
        return fail(GOLHIP_ERANGE, "rule %s needs %zu bytes, the buffer holds %llu", s.c_str(), s.size() + 1,
                    (unsigned long long)cap);
    memcpy(out, s.c_str(), s.size() + 1);
    return GOLHIP_OK;
}

int golhip_rule_parse_ex(const char *text, uint32_t *birth, uint32_t *survive, int32_t *topology, int32_t *bw,
                         int32_t *bh) {
    if (!text || !birth || !survive || !topology || !bw || !bh) return fail(GOLHIP_EINVAL, "null argument");
    std::string why;
    uint32_t b = 0, s = 0;
    int t = 0, w = 0, hh = 0;
    if (!golrule::parse_ex(text, &b, &s, &t, &w, &hh, &why)) return fail(GOLHIP_EINVAL, "%s", why.c_str());
    *birth = b;
    *survive = s;
    *topology = t == golrule::kPlane ? GOLHIP_TOPOLOGY_PLANE : GOLHIP_TOPOLOGY_TORUS;
    *bw = w;
    *bh = hh;
    return GOLHIP_OK;
}

int golhip_rule_format_ex(uint32_t birth, uint32_t survive, int32_t topology, int32_t bw, int32_t bh, char *out,
                          uint64_t cap) {
    if (!out) return fail(GOLHIP_EINVAL, "out is null");
    if (birth > golrule::kMaskAll || survive > golrule::kMaskAll)
        return fail(GOLHIP_EINVAL, "rule masks 0x%x / 0x%x above 0x1FF", birth, survive);
    if (topology != GOLHIP_TOPOLOGY_TORUS && topology != GOLHIP_TOPOLOGY_PLANE)
        return fail(GOLHIP_EINVAL, "topology %d (0: torus, 1: plane)", topology);
    if (bw < 0 || bh < 0 || (bw == 0) != (bh == 0))
        return fail(GOLHIP_EINVAL, "bounds %d x %d: both at least 1, or both 0 for none", bw, bh);
    if (topology == GOLHIP_TOPOLOGY_PLANE && bw == 0) return fail(GOLHIP_EINVAL, "a plane needs its bounds");
    const std::string s =
        golrule::format_ex(birth, survive, topology == GOLHIP_TOPOLOGY_PLANE ? golrule::kPlane : golrule::kTorus, bw, bh);
    if (s.size() + 1 > cap)
        return fail(GOLHIP_ERANGE, "rule %s needs %zu bytes, the buffer holds %llu", s.c_str(), s.size() + 1,
                    (unsigned long long)cap);
    memcpy(out, s.c_str(), s.size() + 1);
    return GOLHIP_OK;
}

int golhip_set_topology(golhip_t h, int32_t topology) {
    if (int rc = check(h)) return rc;
    if (topology != GOLHIP_TOPOLOGY_TORUS && topology != GOLHIP_TOPOLOGY_PLANE)
        return fail(GOLHIP_EINVAL, "topology %d (0: torus, 1: plane)", topology);
    std::lock_guard<std::mutex> g(h->mu);
    const bool plane = topology == GOLHIP_TOPOLOGY_PLANE;
    if (plane && h->ringed())
        return fail(GOLHIP_EINVAL, "a bounded plane on a handle with a communicator: a ring runs the torus only");
    if (plane && h->pad_mode == 1)
        return fail(GOLHIP_EINVAL, "a bounded plane on a handle with golhip_set_pad_step 1: the padded torus copies "
                                   "columns across the row seam, and a plane has none");
    h->plane = plane;
    for (int &c : h->auto_rpw) c = 0;  // the automatic rows per wave are the kernel's
    return GOLHIP_OK;
}

int golhip_topology(golhip_t h, int32_t *topology) {
    if (int rc = check(h)) return rc;
    if (!topology) return fail(GOLHIP_EINVAL, "null output");
    std::lock_guard<std::mutex> g(h->mu);
    *topology = h->plane ? GOLHIP_TOPOLOGY_PLANE : GOLHIP_TOPOLOGY_TORUS;
    return GOLHIP_OK;
}

int golhip_set_rule(golhip_t h, uint32_t birth, uint32_t survive) {
    if (int rc = check(h)) return rc;
    if (birth > golrule::kMaskAll || survive > golrule::kMaskAll)
        return fail(GOLHIP_EINVAL, "rule masks 0x%x / 0x%x above 0x1FF", birth, survive);
    std::lock_guard<std::mutex> g(h->mu);
    const bool conway = birth == golrule::kConwayBirth && survive == golrule::kConwaySurvive;
    if (h->ringed() && !conway)
        return fail(GOLHIP_EINVAL, "rule %s on a handle with a communicator: a ring runs Conway's B3/S23 only",
                    golrule::format(birth, survive).c_str());
    h->birth = birth;
    h->survive = survive;
    if (h->wide) {  // the padded torus / strip steps this handle's turns
        h->wide->birth = birth;
        h->wide->survive = survive;
        for (int &c : h->wide->auto_rpw) c = 0;
    }
    for (int &c : h->auto_rpw) c = 0;  // the automatic rows per wave are the kernel's
    return GOLHIP_OK;
}

int golhip_rule(golhip_t h, uint32_t *birth, uint32_t *survive) {
    if (int rc = check(h)) return rc;
    if (!birth || !survive) return fail(GOLHIP_EINVAL, "null output");
    std::lock_guard<std::mutex> g(h->mu);
    *birth = h->birth;
    *survive = h->survive;
    return GOLHIP_OK;
}

int golhip_set_rule_flips(golhip_t h, int32_t mode) {
    if (int rc = check(h)) return rc;
    if (mode != 0 && mode != 1) return fail(GOLHIP_EINVAL, "rule_flips mode %d (0: per turn, 1: fused)", mode);
    std::lock_guard<std::mutex> g(h->mu);
    h->rule_flips = mode;
    return GOLHIP_OK;
}

int golhip_rule_flips(golhip_t h, int32_t *mode) {
    if (int rc = check(h)) return rc;
    if (!mode) return fail(GOLHIP_EINVAL, "null output");
    std::lock_guard<std::mutex> g(h->mu);
    *mode = h->rule_flips;
    return GOLHIP_OK;
}

}  // extern "C"
