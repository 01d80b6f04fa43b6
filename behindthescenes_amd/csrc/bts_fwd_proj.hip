// PROJ = true instantiations of the fused forward (projected feature map G; the default render path): the software-pipelined
// render kernel (bts_render_kernel.h).  (Field queries on the projected map: bts_query.hip.)
#include "bts_render_kernel.h"
#include "bts_host.h"

namespace bts {
int launch_render_pipelined(const FwdParams& p, int C, int HD, int NB, int grid, hipStream_t s, bool pin) {
  if (p.invalid_wsum || p.invalid_any) return launch_render_pipelined_epi(p, C, HD, NB, grid, s);
  return launch_render_p<false>(p, C, HD, NB, grid, s, pin);
}
}  // namespace bts
