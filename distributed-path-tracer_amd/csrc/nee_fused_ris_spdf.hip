// The variants of k_nee_fused for PTX_NEE_CANDIDATES combined with PTX_NEE_SAMPLER_PDF: nee_fused.hip once more, for its fourth quarter (see
// the end of that file).
#define PTX_NEE_FUSED_RIS_TU 1
#define PTX_NEE_FUSED_SPDF_TU 1
#include "nee_fused.hip"
