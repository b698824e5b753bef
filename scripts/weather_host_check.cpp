// Stand-alone host program for csrc/weather.h (the per-env weather's validation and record building): built
// with the host sanitizers and run once on a CPU, no device and no Python.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -o weather_host_check scripts/weather_host_check.cpp
//   ./weather_host_check
//
// It walks every branch of the header: each refusal, ragged and whole tile counts, both ends of each range,
// and the tile-ordered layout against weather_record() env by env.  Exit status 0 and "ok" when all hold.
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../heli-gym_amd/csrc/weather.h"

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                            \
        }                                                          \
    } while (0)

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // validation
    CHECK(hgw::check_weather(hg_weather{0.f, 0.f, 0.f}) == nullptr);
    CHECK(hgw::check_weather(hg_weather{7.f, -720.f, 1e6f}) == nullptr);
    const hg_weather bad[] = {{nan, 0, 0}, {0, nan, 0}, {0, 0, nan}, {inf, 0, 0}, {0, -inf, 0}, {0, 0, inf},
                              {-0.001f, 0, 0}, {7.001f, 0, 0}, {1, 0, -1e-3f}};
    for (const hg_weather& w : bad) CHECK(hgw::check_weather(w) != nullptr);

    // the constants of the airframe's own ENV block, in both precisions
    const hgw::WindConst<float> cf = hgw::wind_constants<float>(45.0, 20.0, 1.0);
    const hgw::WindConst<double> cd = hgw::wind_constants<double>(45.0, 20.0, 1.0);
    CHECK(cf.wm[2] == 0.f && cd.wm[2] == 0.0 && cf.turb_level == 1.f);
    CHECK(cf.wm[0] == (float)cd.wm[0] && cf.sigma_low == (float)cd.sigma_low);
    CHECK(cf.tep_row[0] == 1.f);
    hg::Params<float> P;
    memset(&P, 0, sizeof(P));
    hgw::set_wind(P, cf);
    CHECK(P.wm[1] == cf.wm[1] && P.tep_row[12] == cf.tep_row[12] && P.w20 == cf.w20);

    // records: sizes around the tile, every env against weather_record()
    for (int64_t n : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)200, (int64_t)4097}) {
        std::vector<hg_weather> w((size_t)n);
        for (int64_t i = 0; i < n; ++i)
            w[(size_t)i] = hg_weather{7.f * (float)(i % 15) / 14.f, 360.f * (float)(i % 37) / 37.f - 90.f, (float)(i % 41)};
        std::vector<float> rec, tep, wind;
        const char* why = nullptr;
        CHECK(hgw::build_records(w.data(), n, rec, tep, wind, &why) == -1 && why == nullptr);
        const int64_t np = hgw::padded_envs(n);
        CHECK(np % 64 == 0 && np >= n && np < n + 64);
        CHECK((int64_t)rec.size() == np * 8 && (int64_t)tep.size() == np * 16 && (int64_t)wind.size() == n * 3);
        for (int64_t i = 0; i < np; ++i) {
            float r[8] = {0}, t[16] = {0};
            if (i < n) hgw::weather_record(w[(size_t)i], r, t);
            const float* tile = &rec[(size_t)(i / 64) * 64 * 8];
            for (int k = 0; k < 4; ++k) {
                CHECK(tile[(i % 64) * 4 + k] == r[k]);
                CHECK(tile[(64 + i % 64) * 4 + k] == r[4 + k]);
            }
            CHECK(memcmp(&tep[(size_t)i * 16], t, sizeof(t)) == 0);
            if (i < n) CHECK(wind[(size_t)i * 3] == r[0] && wind[(size_t)i * 3 + 1] == r[1] && wind[(size_t)i * 3 + 2] == 0.f);
        }
        // a refused env is named, and nothing is built past it
        if (n > 2) {
            w[(size_t)(n - 2)].turb_level = 9.f;
            std::vector<float> r2, t2, w2;
            CHECK(hgw::build_records(w.data(), n, r2, t2, w2, &why) == n - 2 && why != nullptr);
            CHECK(r2.empty() && t2.empty() && w2.empty());
        }
    }
    // the TEP row at both ends and between two levels: inside the table's rows
    for (float lvl : {0.f, 0.5f, 1.f, 3.25f, 6.999f, 7.f}) {
        float r[8], t[16];
        hgw::weather_record(hg_weather{lvl, 10.f, 5.f}, r, t);
        CHECK(r[5] == lvl && t[13] == 0.f && t[15] == 0.f);
        for (int k = 1; k < 13; ++k) CHECK(t[k] >= 0.f && t[k] <= 31.0f);
    }
    printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
