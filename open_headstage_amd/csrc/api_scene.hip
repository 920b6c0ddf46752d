// api_scene.hip -- ohs_scene_* (include/ohs_scene.h): thin shims over the batch object of this library's own copy of the code.
// Linked into libohs_scene.so only; libohs_hip.so does not contain this unit.
#include "../../include/ohs_hip.h"
#include "../../include/ohs_scene.h"
#include "host_internal.h"

#include <new>

static_assert(OHS_SCENE_OK == OHS_OK && OHS_SCENE_ERR_INVALID_ARG == OHS_ERR_INVALID_ARG && OHS_SCENE_ERR_NO_DEVICE == OHS_ERR_NO_DEVICE &&
              OHS_SCENE_ERR_HIP == OHS_ERR_HIP && OHS_SCENE_ERR_ALLOC == OHS_ERR_ALLOC, "ohs_scene.h restates ohs_hip.h's status codes");

struct ohs_scene {
    ohs_batch *b = nullptr;     // never handed out
};

static int scene_null(const char *what)
{
    ohsint_set_error(what);
    return OHS_ERR_INVALID_ARG;
}

extern "C" {

int ohs_scene_create(int device, size_t n_streams, size_t num_bands, ohs_scene **out)
{
    if (!out) return scene_null("out is NULL");
    *out = nullptr;
    ohs_scene *sc = new (std::nothrow) ohs_scene();
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

void ohs_scene_destroy(ohs_scene *sc)
{
    if (!sc) return;
    ohs_batch_destroy(sc->b);
    delete sc;
}

const char *ohs_scene_status_string(int status) { return ohs_status_string(status); }
const char *ohs_scene_last_error(void) { return ohs_last_error(); }

int ohs_scene_set_direction_irs(ohs_scene *sc, size_t n_dirs, const float *irs, size_t len)
{
    if (!sc) return scene_null("scene is NULL");
    return ohsint_batch_set_object_dirs(sc->b, n_dirs, irs, len);
}

int ohs_scene_process(ohs_scene *sc, const float *d_in, float *d_out, size_t n_blocks, size_t in_stream_stride,
                      size_t in_channel_stride, size_t out_stream_stride, size_t out_channel_stride, size_t n_objects,
                      size_t seg_blocks, const unsigned *dir_idx, const float *obj_gain, size_t idx_stride,
                      const unsigned *prev_idx, const float *prev_gain, int switch_mode, void *hip_stream)
{
    if (!sc) return scene_null("scene is NULL");
    return ohsint_batch_process_objects(sc->b, d_in, d_out, n_blocks, in_stream_stride, in_channel_stride, out_stream_stride,
                                        out_channel_stride, n_objects, seg_blocks, dir_idx, obj_gain, idx_stride, prev_idx, prev_gain,
                                        switch_mode, hip_stream);
}

int ohs_scene_set_gain(ohs_scene *sc, float gain)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_set_gain(sc->b, gain);
}

int ohs_scene_set_eq_band_coeffs(ohs_scene *sc, size_t band, const float coeffs[5], int enabled)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_set_eq_band_coeffs(sc->b, band, coeffs, enabled);
}

int ohs_scene_set_eq_enabled(ohs_scene *sc, int eq_enable)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_set_eq_enabled(sc->b, eq_enable);
}

int ohs_scene_set_flush_denormals(ohs_scene *sc, int mode)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_set_flush_denormals(sc->b, mode);
}

int ohs_scene_reset(ohs_scene *sc)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_reset(sc->b);
}

int ohs_scene_sync(ohs_scene *sc, void *hip_stream)
{
    if (!sc) return scene_null("scene is NULL");
    return ohs_batch_sync(sc->b, hip_stream);
}

int ohs_scene_last_launch(const ohs_scene *sc, int *n_pairs, int *ranges_per_stream, unsigned long long *fading_passes)
{
    if (!sc) return scene_null("scene is NULL");
    return ohsint_batch_last_objects_launch(sc->b, n_pairs, ranges_per_stream, fading_passes);
}

}  // extern "C"
