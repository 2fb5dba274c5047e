// The variants of k_nee_shade for scenes with punctual lights (ptx_scene_set_punctual_lights): nee.hip once more, for its second half
// (see the head of that file). A translation unit of its own, as nee_fused_ris.hip is, so that the build stays parallel.
#define PTX_NEE_PUNCTUAL_TU 1
#include "nee.hip"
