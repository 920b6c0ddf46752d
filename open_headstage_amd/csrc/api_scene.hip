// api_scene.hip -- ohs_scene_* (include/ohs_scene.h): the scene surface's bodies (api_scene_bodies.inc) under their first names.
// Linked into libohs_scene.so only; libohs_hip.so does not contain this unit.
#include "../../include/ohs_hip.h"
#include "../../include/ohs_scene.h"
#include "host_internal.h"

static_assert(OHS_SCENE_OK == OHS_OK && OHS_SCENE_ERR_INVALID_ARG == OHS_ERR_INVALID_ARG && OHS_SCENE_ERR_NO_DEVICE == OHS_ERR_NO_DEVICE &&
              OHS_SCENE_ERR_HIP == OHS_ERR_HIP && OHS_SCENE_ERR_ALLOC == OHS_ERR_ALLOC, "ohs_scene.h restates ohs_hip.h's status codes");

#define OHS_SCENE_T ohs_scene
#define OHS_SCENE_FN(name) ohs_scene_##name
#include "api_scene_bodies.inc"
