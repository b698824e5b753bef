// The wind model's constants of one weather (turbulence level, mean wind direction and speed), host only.
// derive() forms the handle-wide ones with wind_constants(); hg_set_weather forms one record per env with
// the same function, so an env given the airframe's own weather steps with the handle's bits.
#ifndef HELIGYM_AMD_WEATHER_H
#define HELIGYM_AMD_WEATHER_H
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/heligym_amd.h"
#include "physics.h"

namespace hgw {

constexpr double kD2R = 3.14159265358979323846 / 180.0;

// the fields of hg::Params<R> a weather decides, under their names there
template <typename R>
struct WindConst {
    R wm[3], wind_dir_cos, wind_dir_sin, w20, sigma_low, turb_level;
    R tep_row[13];
};

// wind_dynamics.py:21-28, 56.  QUIRK: the mean wind's components go through an fp32 cos / sin (the reference
// builds them from a float32 array), the turbulence axes' direction through the fp64 ones.
template <typename R>
WindConst<R> wind_constants(double wind_dir_deg, double wind_spd, double turb_lvl) {
    WindConst<R> c;
    const double wdir = wind_dir_deg * kD2R;
    c.wm[0] = (R)(wind_spd * (double)(float)cos(wdir));
    c.wm[1] = (R)(wind_spd * (double)(float)sin(wdir));
    c.wm[2] = (R)0;
    c.wind_dir_cos = (R)cos(wdir);
    c.wind_dir_sin = (R)sin(wdir);
    const double w20 = turb_lvl / 7.0 * 88.61;
    c.w20 = (R)w20;
    c.sigma_low = (R)(0.1 * w20);
    c.turb_level = (R)turb_lvl;
    hg::tep_row_values(c.turb_level, c.tep_row);
    return c;
}

template <typename R>
void set_wind(hg::Params<R>& P, const WindConst<R>& c) {
    for (int k = 0; k < 3; ++k) P.wm[k] = c.wm[k];
    P.wind_dir_cos = c.wind_dir_cos;
    P.wind_dir_sin = c.wind_dir_sin;
    P.w20 = c.w20;
    P.sigma_low = c.sigma_low;
    P.turb_level = c.turb_level;
    for (int k = 0; k < 13; ++k) P.tep_row[k] = c.tep_row[k];
}

// Per-env records as the step kernels read them.  Two 16-byte words per env, kept tile by tile like the
// state (a wave's 64 first words, then its 64 second words), padded to whole tiles; and one 64-byte TEP row
// per env, padded the same way:
//   word 0 {wm north, wm east, cos dir, sin dir}   word 1 {sigma_low, turb_level, 0, 0}
constexpr int kRecFloats = 8;    // per env
constexpr int kTepFloats = 16;   // per env: 13 values, 3 zeros
constexpr int64_t kTile = 64;

inline int64_t padded_envs(int64_t n) { return (n + kTile - 1) / kTile * kTile; }

// nullptr, or what is wrong with the weather
inline const char* check_weather(const hg_weather& w) {
    if (!isfinite(w.turb_level) || !isfinite(w.wind_dir_deg) || !isfinite(w.wind_spd)) return "a non-finite value";
    if (w.turb_level < 0.f || w.turb_level > 7.f) return "turb_level outside [0, 7]";
    if (w.wind_spd < 0.f) return "a negative wind_spd";
    return nullptr;
}

// one env's record and TEP row: the values of derive<float>() for an airframe with this ENV block
inline void weather_record(const hg_weather& w, float record[kRecFloats], float tep_row[kTepFloats]) {
    const WindConst<float> c = wind_constants<float>((double)w.wind_dir_deg, (double)w.wind_spd, (double)w.turb_level);
    record[0] = c.wm[0];
    record[1] = c.wm[1];
    record[2] = c.wind_dir_cos;
    record[3] = c.wind_dir_sin;
    record[4] = c.sigma_low;
    record[5] = c.turb_level;
    record[6] = 0.f;
    record[7] = 0.f;
    for (int k = 0; k < 13; ++k) tep_row[k] = c.tep_row[k];
    for (int k = 13; k < kTepFloats; ++k) tep_row[k] = 0.f;
}

// The handle's images: rec [padded][8] in tile order, tep [padded][16], and the trims' winds [n][3] (the
// mean wind in fp32).  Returns the first env whose weather is refused (its reason in *why), or -1.
inline int64_t build_records(const hg_weather* w, int64_t n, std::vector<float>& rec, std::vector<float>& tep,
                             std::vector<float>& wind, const char** why) {
    for (int64_t i = 0; i < n; ++i) {
        const char* bad = check_weather(w[i]);
        if (bad) {
            if (why) *why = bad;
            return i;
        }
    }
    const int64_t np = padded_envs(n);
    rec.assign((size_t)np * kRecFloats, 0.f);
    tep.assign((size_t)np * kTepFloats, 0.f);
    wind.assign((size_t)n * 3, 0.f);
    for (int64_t i = 0; i < n; ++i) {
        float r[kRecFloats];
        weather_record(w[i], r, &tep[(size_t)i * kTepFloats]);
        float* t = &rec[(size_t)(i / kTile) * kTile * kRecFloats];
        const int64_t l = i % kTile;
        for (int k = 0; k < 4; ++k) {
            t[l * 4 + k] = r[k];
            t[(kTile + l) * 4 + k] = r[4 + k];
        }
        wind[(size_t)i * 3 + 0] = r[0];
        wind[(size_t)i * 3 + 1] = r[1];
    }
    return -1;
}

}  // namespace hgw
#endif
