// The variants of k_nee_fused for scenes with punctual lights (ptx_scene_set_punctual_lights), PTX_NEE_CANDIDATES: nee_fused.hip once more
// (see the end of that file). A translation unit of its own, as nee_fused_ris.hip is, so that the build stays parallel.
#define PTX_NEE_FUSED_PUN_TU 1
#define PTX_NEE_FUSED_RIS_TU 1
#include "nee_fused.hip"
