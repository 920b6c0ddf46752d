// speakers.cpp -- the wiring the reference plans but does not have: the plugin's four speaker-angle parameters
// (CLAP ids az_l / el_l / az_r / el_r, src/lib.rs:120-128; their smoothed values are discarded at :1170-1173) ->
// MySofa::get_hrtf_irs (src/sofa/loader.rs:136-199) for each speaker -> four set_ir calls
// (github_issues/sofa_implement_logic_select_extract_hrirs.md:5: "select the nearest available HRTF measurement ...
// extract the four required HRIRs (LSL, LSR, RSL, RSR)").  Host-only C++ on top of the SOFA reader.
#include "../../include/ohs_hip.h"
#include "host_internal.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace ohs_host {

// one speaker at the plugin's (az, el): its left-ear and right-ear responses
static int one_speaker_irs(const ohs_sofa *sofa, float az, float el, float radius_m, float fs, std::vector<float> out[2])
{
    size_t M = 0, R = 0, N = 0;
    float file_fs = 0.f;
    int rc = ohs_sofa_info(sofa, &M, &R, &N, &file_fs);
    if (rc) return rc;
    std::vector<float> ear[2] = {std::vector<float>(N), std::vector<float>(N)};
    float dl = 0.f, dr = 0.f;
    rc = ohs_sofa_get_hrtf_irs(sofa, -az, el, radius_m, ear[0].data(), ear[1].data(), N, &dl, &dr);
    if (rc) return rc;
    for (int e = 0; e < 2; ++e) {
        std::vector<float> &dst = out[e];
        if (fs > 0.f && std::fabs(fs - file_fs) > 1e-3f) {
            size_t n_out = 0;
            rc = ohs_sofa_resample_ir(ear[e].data(), N, file_fs, fs, nullptr, 0, &n_out);
            if (rc) return rc;
            dst.assign(n_out, 0.0f);
            rc = ohs_sofa_resample_ir(ear[e].data(), N, file_fs, fs, dst.data(), dst.size(), &n_out);
            if (rc) return rc;
        } else {
            dst = ear[e];
        }
    }
    return OHS_OK;
}

// The left speaker's (left-ear, right-ear) responses become Lsl / Lsr, the right speaker's Rsl / Rsr.
// Angles are the PLUGIN's: degrees, azimuth positive to the RIGHT (the editor draws a speaker at x = sin(az),
// src/ui/speaker_visualizer.rs:51-54; defaults az_l = -30, az_r = +30, src/lib.rs:429-432), elevation up.  SOFA / AES69
// azimuth is counter-clockwise (positive = left), hence the sign.  fs > 0: every response resampled from the file's
// rate to fs when they differ by more than 1e-3 Hz (libmysofa does this inside mysofa_open, loader.rs:83-90); fs <= 0:
// the file's own samples.
int speaker_irs(const ohs_sofa *sofa, float az_l, float el_l, float az_r, float el_r, float radius_m, float fs,
                std::vector<float> out[4])
{
    const int rc = one_speaker_irs(sofa, az_l, el_l, radius_m, fs, out);
    return rc ? rc : one_speaker_irs(sofa, az_r, el_r, radius_m, fs, out + 2);
}

}  // namespace ohs_host

extern "C" {

// the four responses themselves, for hosts that want them without a device (and for the CPU test suite)
int ohs_sofa_speaker_irs(const ohs_sofa *sofa, float az_l, float el_l, float az_r, float el_r, float radius_m, float fs,
                         float *const out[4], size_t capacity, size_t lens[4])
{
    if (!sofa || !lens) { ohsint_set_error("NULL argument"); return OHS_ERR_INVALID_ARG; }
    std::vector<float> irs[4];
    const int rc = ohs_host::speaker_irs(sofa, az_l, el_l, az_r, el_r, radius_m, fs, irs);
    if (rc) return rc;
    for (int p = 0; p < 4; ++p) {
        lens[p] = irs[p].size();
        if (out && out[p])
            for (size_t i = 0; i < irs[p].size() && i < capacity; ++i) out[p][i] = irs[p][i];
    }
    return OHS_OK;
}

// K speakers for ohs_batch_set_layout_irs: speaker c is what speaker_irs makes of one speaker at (az[c], el[c]) -- the same lookup,
// the same resampling --, its two ears at out[c][0] and out[c][1]
int ohs_sofa_layout_irs(const ohs_sofa *sofa, size_t n_channels, const float *az_deg, const float *el_deg, float radius_m, float fs,
                        float *out, size_t len, size_t *max_len)
{
    if (!sofa || !az_deg || !el_deg || !max_len) { ohsint_set_error("NULL argument"); return OHS_ERR_INVALID_ARG; }
    if (n_channels == 0 || n_channels > 16) { ohsint_set_error("n_channels must be 1 .. 16"); return OHS_ERR_INVALID_ARG; }
    std::vector<std::vector<float>> all(2 * n_channels);
    size_t longest = 0;
    for (size_t c = 0; c < n_channels; ++c) {
        std::vector<float> irs[2];
        const int rc = ohs_host::one_speaker_irs(sofa, az_deg[c], el_deg[c], radius_m, fs, irs);
        if (rc) return rc;
        for (int e = 0; e < 2; ++e) {
            longest = std::max(longest, irs[e].size());
            all[2 * c + e] = std::move(irs[e]);
        }
    }
    *max_len = longest;
    if (!out) return OHS_OK;
    if (len < longest) { ohsint_set_error("len is smaller than the longest response"); return OHS_ERR_INVALID_ARG; }
    for (size_t r = 0; r < 2 * n_channels; ++r) {
        float *dst = out + r * len;
        for (size_t i = 0; i < len; ++i) dst[i] = i < all[r].size() ? all[r][i] : 0.0f;
    }
    return OHS_OK;
}

// A table of layouts for ohs_batch_set_layout_schedule_irs, one per head yaw: set j is ohs_sofa_layout_irs with every speaker at
// az[c] - yaw[j] (the head turns to the right by yaw, positive like the azimuth, so the room turns to the left around it), wrapped
// into [-180, 180).  Two passes over that function: the lengths first, then every set at the longest.
int ohs_sofa_layout_yaw_irs(const ohs_sofa *sofa, size_t n_channels, const float *az_deg, const float *el_deg, float radius_m, float fs,
                            size_t n_yaws, const float *yaw_deg, float *out, size_t len, size_t *needed_len)
{
    if (!sofa || !az_deg || !el_deg || !yaw_deg || !needed_len) { ohsint_set_error("NULL argument"); return OHS_ERR_INVALID_ARG; }
    if (n_channels == 0 || n_channels > 16) { ohsint_set_error("n_channels must be 1 .. 16"); return OHS_ERR_INVALID_ARG; }
    if (n_yaws == 0 || n_yaws > 65536) { ohsint_set_error("n_yaws must be 1 .. 65536"); return OHS_ERR_INVALID_ARG; }
    std::vector<float> az(n_yaws * n_channels);
    size_t longest = 0;
    for (size_t j = 0; j < n_yaws; ++j) {
        float *a = &az[j * n_channels];
        for (size_t c = 0; c < n_channels; ++c) {
            const float d = az_deg[c] - yaw_deg[j];
            a[c] = d - 360.0f * std::floor((d + 180.0f) / 360.0f);
        }
        size_t n = 0;
        const int rc = ohs_sofa_layout_irs(sofa, n_channels, a, el_deg, radius_m, fs, nullptr, 0, &n);
        if (rc) return rc;
        longest = std::max(longest, n);
    }
    *needed_len = longest;
    if (!out) return OHS_OK;
    if (len < longest) { ohsint_set_error("len is smaller than the longest response"); return OHS_ERR_INVALID_ARG; }
    for (size_t j = 0; j < n_yaws; ++j) {
        size_t n = 0;
        const int rc = ohs_sofa_layout_irs(sofa, n_channels, &az[j * n_channels], el_deg, radius_m, fs, out + j * n_channels * 2 * len, len, &n);
        if (rc) return rc;
    }
    return OHS_OK;
}

}  // extern "C"
