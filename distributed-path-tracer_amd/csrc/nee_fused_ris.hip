// The variants of k_nee_fused for PTX_NEE_CANDIDATES (the light sample chosen among M candidates): nee_fused.hip once more, for its third
// quarter (see the end of that file). A translation unit of its own, as nee_fused_spdf.hip is, so that the build stays parallel.
#define PTX_NEE_FUSED_RIS_TU 1
#include "nee_fused.hip"
