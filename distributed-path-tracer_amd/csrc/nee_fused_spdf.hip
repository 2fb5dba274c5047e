// The variants of k_nee_fused for PTX_NEE_SAMPLER_PDF: nee_fused.hip once more, for its second half (see the end of that file). A translation
// unit of its own so that the 36 flagged variants compile next to the 36 unflagged ones instead of after them.
#define PTX_NEE_FUSED_SPDF_TU 1
#include "nee_fused.hip"
