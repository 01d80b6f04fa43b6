// Host side of bts_render_bwd: path choice, workspace layout and the launch of the lane = sample passes.  Plain MLP and K <= 64: the
// gate-bit passes of bts_bwd_rows.hip; ResnetBlockFC layers (RE10K) or longer rays: the row passes of bts_bwd_blocks.hip.  This file
// holds no device code.
//
// What torch.autograd would do for nerf.py:283-299 + models_bts.py:266-338 + resnetfc.py:132-184 of the reference.
#include "bts_bwd.h"
#include "bts_host.h"
#include <cstdlib>

namespace bts {

// plain MLP and at most one wave of samples per ray: the gate-bit passes of bts_bwd_rows.hip; ResnetBlockFC layers (RE10K) and K > 64:
// the row passes of bts_bwd_blocks.hip
static bool bits_path(const BtsFieldCfg* cfg, const BtsRenderArgs* a) { return cfg->n_blocks == 0 && a->K <= 64; }

// workspace = what the passes hand each other per sample.  Gate-bit path: g_s (one float) + the relu gates as bits, once per sample
// and once per channel -- 20 bytes at d_hidden 64.  Row path: the gradient row at lin_in's output (4 d_hidden bytes) + g_s.
// + pass C's slot copies of dW_pe (bts_bwd.h: kFlushSlots x 40 x d_hidden floats, 80 KB at d_hidden 64), behind the per-sample part
static size_t flush_bytes(const BtsFieldCfg* cfg) { return sizeof(float) * kFlushSlots * kFlushRows * (size_t)cfg->d_hidden; }
size_t render_bwd_workspace_impl(const BtsFieldCfg* cfg, const BtsRenderArgs* a) {
  const size_t rays = (size_t)cfg->n * (size_t)a->rays_per_sample;
  // gate-bit path: g_s + the per-sample masks, rounded up to 8 bytes (the per-channel masks behind them are read as 64-bit words)
  const size_t bits = align16(((rays * (size_t)a->K * (1 + (size_t)cfg->d_hidden / 32) + 1) & ~(size_t)1) * sizeof(float) +
                              rays * 2 * (size_t)cfg->d_hidden * sizeof(float)) + flush_bytes(cfg);
  const size_t rows = align16(rays * (size_t)a->K * ((size_t)cfg->d_hidden + 1) * sizeof(float)) + flush_bytes(cfg);
  return bits_path(cfg, a) ? bits : rows;
}

// where pass C's slot copies sit inside a workspace (the tail of either layout), for a caller that zeroes them itself
void render_bwd_flush_region(const BtsFieldCfg* cfg, const BtsRenderArgs* a, void* workspace, float** ptr, size_t* bytes) {
  const size_t total = render_bwd_workspace_impl(cfg, a);
  *bytes = flush_bytes(cfg);
  *ptr = reinterpret_cast<float*>(static_cast<char*>(workspace) + (total - *bytes));
}

int render_bwd_impl(const BtsFieldCfg* cfg, const BtsFieldTensors* t, const BtsRenderArgs* a, const BtsRenderGrads* g, void* workspace,
                    hipStream_t s, bool flush_clean) {
  BwdParams bp;
  bp.flush_clean = flush_clean;
  bp.f = make_params(cfg, t);
  bp.f.rays = a->rays, bp.f.z_samp = a->z_samp;
  bp.f.Bp = a->rays_per_sample, bp.f.K = a->K, bp.f.hard_cap = a->hard_alpha_cap, bp.f.white_bkgd = a->white_bkgd;
  bp.f.sigma_raw = a->sigma_raw, bp.f.trans = a->trans, bp.f.sigma_noise = a->sigma_noise;
  bp.f.rgb_samps = a->rgb_samps;   // optional INPUT here: the forward's per-sample colours (else they are recomputed)
  bp.f.tiles_per_sample = (a->rays_per_sample + 255) / 256;
  bp.g_rgb = g->g_rgb, bp.g_depth = g->g_depth, bp.g_weights = g->g_weights, bp.g_alphas = g->g_alphas;
  bp.d_proj = g->d_proj_nhwc, bp.d_mlp = g->d_mlp_params, bp.d_empty_proj = g->d_empty_proj;
  bp.gh_ws = nullptr;   // (no reader: see BwdParams)
  bp.gs_ws = nullptr, bp.mask_ws = nullptr, bp.pmask_ws = nullptr, bp.flush_ws = nullptr;
#ifdef BTS_TICKS
  bp.ticks = nullptr;
  if (const char* e = getenv("BTS_DBG_PTR")) bp.ticks = (unsigned long long*)strtoull(e, nullptr, 0);   // diagnostic build only
#endif
  bp.tiles = bp.d_proj ? g->d_proj_tiles : nullptr;
  bp.tiles_per_img = (int)map_tiles(cfg->H, cfg->W, cfg->feat_shift);
  bp.tile_tw = tile_cols(cfg->H >> cfg->feat_shift, cfg->W >> cfg->feat_shift, cfg->tile_blocks);
  bp.f.lpr = 64, bp.f.groups = (long)cfg->n * a->rays_per_sample;
  if (bp.f.groups > 0x7FF00000L) {
    set_error("%s: too many rays in one call (%ld)", "bts_render_bwd", bp.f.groups);
    return BTS_E_UNSUPPORTED;
  }
  // the RE10K model at its own sample count (32 < K <= 48, exp_re10k.yaml: 48): four rays in three wave iterations (rowsb_kernel<PK>)
  const bool pack48 = Re10kShape::is(cfg->C, cfg->d_hidden, cfg->n_blocks) && a->K > 32 && a->K <= 48 && a->rays_per_sample % 4 == 0;
  if (pack48) bp.f.lpr = 48, bp.f.groups /= 4;
  const int grid = render_grid(bp.f);
  bp.f.chunk_log2 = render_chunk_log2(grid, bp.f.groups);
  const size_t samples = (size_t)cfg->n * a->rays_per_sample * a->K;
  int rc;
  if (bits_path(cfg, a)) {
    bp.gs_ws = static_cast<float*>(workspace);
    bp.mask_ws = reinterpret_cast<unsigned*>(bp.gs_ws + samples);
    const size_t head = (samples * (1 + (size_t)cfg->d_hidden / 32) + 1) & ~(size_t)1;   // dwords, even: the 64-bit masks stay 8-byte aligned
    bp.pmask_ws = reinterpret_cast<uint2*>(bp.gs_ws + head);
    bp.flush_ws = reinterpret_cast<float*>(static_cast<char*>(workspace) +
                                           align16((head + (size_t)cfg->n * a->rays_per_sample * 2 * (size_t)cfg->d_hidden) * sizeof(float)));
    rc = launch_bwd_rows(bp, cfg->C, cfg->d_hidden, cfg->n, grid, s);
  } else {
    float* u0_ws = static_cast<float*>(workspace);          // (rays, K, d_hidden): rows first, they are read as 16-byte pieces
    bp.gs_ws = u0_ws + samples * (size_t)cfg->d_hidden;     // (rays, K)
    bp.flush_ws = reinterpret_cast<float*>(static_cast<char*>(workspace) + align16(samples * ((size_t)cfg->d_hidden + 1) * sizeof(float)));
    rc = launch_bwd_blocks(bp, u0_ws, cfg->C, cfg->d_hidden, cfg->n_blocks, cfg->n, grid, s);
  }
  if (rc != BTS_E_UNSUPPORTED) return rc;
  set_error("%s: unsupported MLP shape C=%ld d_hidden=%ld n_blocks=%ld", "bts_render_bwd", cfg->C, cfg->d_hidden, cfg->n_blocks);
  return rc;
}

}  // namespace bts
