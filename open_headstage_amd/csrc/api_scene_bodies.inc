// api_scene_bodies.inc -- the bodies of the scene surface, once: thin shims over the batch object of the including library's own copy
// of the code.  api_scene.hip compiles them as ohs_scene_* (include/ohs_scene.h, libohs_scene.so), api_scene2.hip as ohs_scene2_*
// (include/ohs_scene2.h, libohs_scene2.so).  The including unit defines
//   OHS_SCENE_T          the handle's struct tag (ohs_scene / ohs_scene2)
//   OHS_SCENE_FN(name)   the entry's name (ohs_scene_##name / ohs_scene2_##name)
//   OHS_SCENE_OWN_LAST_LAUNCH   (optional) the unit brings a last_launch of its own signature
// and has included ohs_hip.h, its own header and host_internal.h.
#include <new>

struct OHS_SCENE_T {
    ohs_batch *b = nullptr;     // never handed out
};

static int scene_null(const char *what)
{
    ohsint_set_error(what);
    return OHS_ERR_INVALID_ARG;
}

extern "C" {

int OHS_SCENE_FN(create)(int device, size_t n_streams, size_t num_bands, OHS_SCENE_T **out)
{
    if (!out) return scene_null("out is NULL");
    *out = nullptr;
    OHS_SCENE_T *sc = new (std::nothrow) OHS_SCENE_T();
    if (!sc) {
        ohsint_set_error("out of host memory");
        return OHS_ERR_ALLOC;
    }
    const int rc = ohs_batch_create(device, n_streams, num_bands, &sc->b);
    if (rc) {
        delete sc;
        return rc;
    }
    *out = sc;
    return OHS_OK;
}

void OHS_SCENE_FN(destroy)(OHS_SCENE_T *sc)
{
    if (!sc) return;
    ohs_batch_destroy(sc->b);
    delete sc;
}

const char *OHS_SCENE_FN(status_string)(int status) { return ohs_status_string(status); }
const char *OHS_SCENE_FN(last_error)(void) { return ohs_last_error(); }

int OHS_SCENE_FN(set_direction_irs)(OHS_SCENE_T *sc, size_t n_dirs, const float *irs, size_t len)
{
    if (!sc) return scene_null("scene is NULL");
    return ohsint_batch_set_object_dirs(sc->b, n_dirs, irs, len);
}

int OHS_SCENE_FN(process)(OHS_SCENE_T *sc, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                      size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                      size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain, size_t idx_stride,
                      const unsigned *prev_idx, const float *prev_gain, int switch_mode, void *hip_stream)
{
    if (!sc) return scene_null("scene is NULL");
    return ohsint_batch_process_objects(sc->b, d_in, d_out, n_blocks, in_stream_stride, in_channel_stride, out_stream_stride,
                                        out_channel_stride, n_objects, seg_blocks, dir_idx, obj_gain, idx_stride, prev_idx, prev_gain,
                                        switch_mode, hip_stream);
}

int OHS_SCENE_FN(set_gain)(OHS_SCENE_T *sc, float gain)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_set_gain(sc->b, gain);
}

int OHS_SCENE_FN(set_eq_band_coeffs)(OHS_SCENE_T *sc, size_t band, const float coeffs[5], int enabled)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_set_eq_band_coeffs(sc->b, band, coeffs, enabled);
}

int OHS_SCENE_FN(set_eq_enabled)(OHS_SCENE_T *sc, int eq_enable)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_set_eq_enabled(sc->b, eq_enable);
}

int OHS_SCENE_FN(set_flush_denormals)(OHS_SCENE_T *sc, int mode)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_set_flush_denormals(sc->b, mode);
}

int OHS_SCENE_FN(reset)(OHS_SCENE_T *sc)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_reset(sc->b);
}

int OHS_SCENE_FN(sync)(OHS_SCENE_T *sc, void *hip_stream)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_sync(sc->b, hip_stream);
}

#ifndef OHS_SCENE_OWN_LAST_LAUNCH
int OHS_SCENE_FN(last_launch)(const OHS_SCENE_T *sc, int *n_pairs, int *ranges_per_stream, unsigned long long *fading_passes)
{
    if (!sc) return scene_null("scene is NULL");
    return ohsint_batch_last_objects_launch(sc->b, n_pairs, ranges_per_stream, fading_passes);
}
#endif

}  // extern "C"
