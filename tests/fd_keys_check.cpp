// Host check of the integer formulas of bcsd_fd_kernel's keys and tag addresses (sd_bcsd_plan.h, namespace sdfx::tmj): the forms
// the kernel evaluates (key_u2, key_off, pad_key) against the forms they replaced (key_u2_ref, tag_off_ref) and against the layout
// restated here:
//   key      t + 2^21 has its mantissa = t in units of 2^-31; q = floor(t) for t in [0, 2^21), clamped to kQD; key = (q << 11) | tag
//   address  tag = 16 chunk + slot -> chunk * 1 032 + 64 slot
//   pads     lane l >= nl, sample i: q = kQD + 1 + 20 l + i, tag = 20 l + i
// out: "ok <check>" or "FAIL <check>: <what>" per check, then "end"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "sd_bcsd_plan.h"

using namespace sdfx;
using namespace sdfx::tmj;

static void words_of(double t, uint32_t* w0, uint32_t* w1) {
    const double s = t + 2097152.0;
    uint64_t b;
    memcpy(&b, &s, sizeof b);
    *w0 = (uint32_t)b;
    *w1 = (uint32_t)(b >> 32);
}

// both forms on the words of every t, with every tag; finite: the key is also compared with the q stated above
static bool keys_equal(const std::vector<double>& ts, bool finite, char* what, size_t cap) {
    for (double t : ts) {
        uint32_t w0, w1;
        words_of(t, &w0, &w1);
        for (uint32_t tag = 0; tag <= kTagMask; ++tag) {
            const uint32_t a = key_u2_ref(w0, w1, tag), b = key_u2(w0, w1, tag);
            if (a != b) {
                snprintf(what, cap, "t = %.17g tag %u: %08x (replaced form) != %08x", t, tag, a, b);
                return false;
            }
            if (finite) {
                // the sum t + 2^21 is rounded to 2^-31: floor of the rounded value
                const double q = std::floor((t + 2097152.0) - 2097152.0);
                const uint32_t qe = q < (double)kQD ? (uint32_t)q : kQD;
                if (b != ((qe << kTagBits) | tag)) {
                    snprintf(what, cap, "t = %.17g tag %u: key %08x, expected q %u", t, tag, b, qe);
                    return false;
                }
            }
        }
    }
    return true;
}

static void report(const char* name, bool ok, const char* what) {
    if (ok) printf("ok %s\n", name);
    else printf("FAIL %s: %s\n", name, what);
}

int main() {
    char what[256] = "";
    const double top = (double)kQD;
    {  // about 10^5 values spread over [1, kQD - 1] (an irrational stride: every fraction), and the exact ends
        std::vector<double> ts = {1.0, top - 1.0, top};
        const int n = 100000;
        const double step = (top - 2.0) / n;
        for (int i = 0; i < n; ++i) ts.push_back(1.0 + step * (i + 0.6180339887498949));
        report("spread", keys_equal(ts, true, what, sizeof what), what);
    }
    {  // within one ulp of an integer and of a half (ulps of t itself, far below the 2^-31 of the sum, and ulps of the sum)
        std::vector<double> ts;
        const double u = std::ldexp(1.0, -31);
        for (double n = 1.0; n <= top; n = n < 64.0 ? n + 1.0 : std::floor(n * 1.37) + 1.0) {
            for (double c : {n, n + 0.5}) {
                if (c > top) continue;
                ts.push_back(c);
                ts.push_back(std::nextafter(c, 0.0));
                ts.push_back(std::nextafter(c, 4.0e6));
                ts.push_back(c - u);
                ts.push_back(c + u);
                ts.push_back(c - u / 2);  // ties of the rounding of the sum
                ts.push_back(c + u / 2);
            }
        }
        for (double c : {top - 1.0, top - 0.5, top}) {
            ts.push_back(std::nextafter(c, 0.0));
            ts.push_back(std::nextafter(c, 4.0e6));
        }
        report("near_integers_and_halves", keys_equal(ts, true, what, sizeof what), what);
    }
    {  // NaN (t of a segment whose samples are all equal) and the infinities: old against new, and NaN's q = 2^20
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        bool ok = keys_equal({nan, -nan, inf, -inf}, false, what, sizeof what);
        uint32_t w0, w1;
        words_of(nan, &w0, &w1);
        if (ok && (key_u2(w0, w1, 5u) != (((1u << 20) << kTagBits) | 5u) || w0 != 0u)) {
            snprintf(what, sizeof what, "NaN: key %08x, u2 %08x", key_u2(w0, w1, 5u), w0);
            ok = false;
        }
        report("nonfinite", ok, what);
    }
    {  // tag addresses: every tag under every q pattern, both forms and the layout; then the tags of every lane with data, for
       // every count of data lanes that occurs (57, 60, 62, 64): inside the tile, no two samples in one place
        bool ok = true;
        for (uint32_t tag = 0; ok && tag <= kTagMask; ++tag)
            for (uint32_t q : {0u, 1u, kQD, kQD + 1u + tag, 0x1fffffu, 0x155555u}) {
                const uint32_t key = (q << kTagBits) | tag, exp = (tag / 16u) * (uint32_t)kChunkStride + 64u * (tag % 16u);
                if (tag_off_ref(tag) != exp || key_off(key) != exp || key_off(tag) != exp) {
                    snprintf(what, sizeof what, "tag %u q %u: %u (replaced form), %u (from the key), layout %u", tag, q, tag_off_ref(tag),
                             key_off(key), exp);
                    ok = false;
                    break;
                }
            }
        for (int nl : {57, 60, 62, 64}) {
            if (!ok) break;
            const uint32_t tile = (uint32_t)chunks_of(kBlock * nl) * (uint32_t)kChunkStride;
            std::vector<char> used(tile / 8u + 8u, 0);
            for (int lane = 0; ok && lane < nl; ++lane)
                for (int i = 0; i < kBlock; ++i) {
                    const uint32_t tag = i < 16 ? 16u * (uint32_t)lane + (uint32_t)i
                                                : 16u * (uint32_t)(nl + tail_chunk(lane)) + (uint32_t)tail_slot(lane) + 4u * (uint32_t)(i - 16);
                    const uint32_t off = key_off((kQD << kTagBits) | tag);
                    if (tag > kTagMask || off != tag_off_ref(tag) || off + 64u > tile || used[off / 8u]) {
                        snprintf(what, sizeof what, "nl %d lane %d sample %d: tag %u at %u (tile %u bytes)", nl, lane, i, tag, off, tile);
                        ok = false;
                        break;
                    }
                    used[off / 8u] = 1;
                    // the row the request tables put there is the sample's
                    if (row_of_slot((int)(tag / 16u), (int)(tag % 16u), nl, kBlock * nl) != kBlock * lane + i) {
                        snprintf(what, sizeof what, "nl %d lane %d sample %d: slot of another row", nl, lane, i);
                        ok = false;
                        break;
                    }
                }
        }
        report("tag_addresses", ok, what);
    }
    {  // pad keys of every lane >= nl: the replaced formula, the fields, above every data key, ascending with the position
        bool ok = true;
        const uint32_t biggest_data = (kQD << kTagBits) | kTagMask;
        for (int nl : {57, 60, 62, 64}) {
            uint32_t prev = biggest_data;
            for (int lane = nl; ok && lane < 64; ++lane)
                for (int i = 0; i < kBlock; ++i) {
                    const uint32_t tag0 = (uint32_t)(kBlock * lane), pad0 = ((kQD + 1u + tag0) << kTagBits) | tag0;
                    const uint32_t old = pad0 + (uint32_t)i * ((1u << kTagBits) + 1u), pk = pad_key(lane, i);
                    const uint32_t pos = (uint32_t)(kBlock * lane + i);
                    if (pk != old || (pk >> kTagBits) != kQD + 1u + pos || (pk & kTagMask) != pos || pk <= prev) {
                        snprintf(what, sizeof what, "nl %d lane %d sample %d: pad %08x, replaced form %08x", nl, lane, i, pk, old);
                        ok = false;
                        break;
                    }
                    prev = pk;
                }
        }
        report("pad_keys", ok, what);
    }
    printf("end\n");
    return 0;
}
