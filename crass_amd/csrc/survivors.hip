// survivors.hip — the ONE translation unit of pass 1's step 2: the wave-per-read survivor search, long reads' light walk and the
// lane-per-read survivor search.  The three are files of their own to read and to edit (about a thousand lines each, nothing in
// one names anything of another but through search_bits.h); they are compiled together because the code the compiler makes for
// k_survivor depends on which kernels share its unit: search_bits.h's helpers are force-inlined and nested, the inliner folds
// them in the order in which the unit's kernels first reach them, and with the light walk and the lane kernel beside it that
// order — and with it every kernel's instruction count and register notes — is the one these kernels were tuned and measured
// with (profiles/NOTES_r23.md has the comparison, unit by unit).  kernels.hip, the seed filters and hints, stands alone.
#include "survivor_wave.hip"
#include "long_light.hip"
#include "survivor_lanes.hip"
