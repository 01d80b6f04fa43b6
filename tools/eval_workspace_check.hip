// Host check of the evaluation workspaces (csrc/bts_host.h: Carver; lidar_bins_layout, occ_eval_layout, bbox_eval_layout, depth_layout,
// nvs_layout): the counted size is where the carved pointers end.  The sibling of tools/loss_workspace_check.hip.
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/eval_workspace_check.hip -o /tmp/eval_workspace_check
//   /tmp/eval_workspace_check          (carves only, launches nothing: needs no GPU)
// The four .hip files are compiled INTO this program, so it calls the layout functions the library calls.
#include "../behindthescenes_amd/csrc/bts_occ.hip"
#include "../behindthescenes_amd/csrc/bts_bbox_occ.hip"
#include "../behindthescenes_amd/csrc/bts_depth_metrics.hip"
#include "../behindthescenes_amd/csrc/bts_nvs_metrics.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace bts {
void set_error(const char*, const char*, long, long, long) {}      // bts_fwd.hip's, not linked here

// [first, last + last_bytes) must be exactly the `bytes - 256` behind the rounded-up workspace pointer, inside the allocation
static int check(const char* what, const Carver& carve, const char* ws, const char* alloc_end, size_t bytes, const void* first, const void* last,
                 size_t last_bytes, const int* shape) {
  const char* base = reinterpret_cast<const char*>(up256((size_t)(uintptr_t)ws));
  const char* end = reinterpret_cast<const char*>(last) + up256(last_bytes);
  const bool ok = carve.bytes() == bytes && first == base && end == base + (bytes - kAlign) && end <= alloc_end;
  if (ok) memset(const_cast<char*>(base), 0x5a, (size_t)(end - base));      // every byte handed out is the caller's
  printf("%-12s (%d, %d, %d, %d) at ..%03zx: %zu bytes %s\n", what, shape[0], shape[1], shape[2], shape[3], (size_t)(uintptr_t)ws & 0xfff, bytes,
         ok ? "ok" : "MISMATCH");
  return ok ? 0 : 1;
}
}  // namespace bts

int main() {
  using namespace bts;
  // P / B, then the layout's own sizes: (T, y_res) for the LiDAR pair, (boxes, ph, pw), (Hg, Wg), (He, We)
  static const int shapes[4][4] = {{1, 1, 1, 1}, {1000, 3, 5, 7}, {4097, 32, 16, 33}, {250000, 20, 192, 640}};
  int bad = 0;
  for (const int* s : shapes) {
    for (int off = 0; off < 2; ++off) {      // once as malloc aligned it, once off by one byte
      {
        const size_t bytes = lidar_bins_bytes(s[1], s[2]);
        char* ws = static_cast<char*>(malloc(bytes + off));
        Carver carve(ws + off);
        const LidarBins b = lidar_bins_layout(carve, s[1], s[2]);
        bad += check("lidar bins", carve, ws + off, ws + off + bytes, bytes, b.bins, b.first, (size_t)s[1] * s[2] * 8, s);
        free(ws);
      }
      {
        Carver count(nullptr);
        occ_eval_layout(count, s[0], s[1], s[2]);
        const size_t bytes = count.bytes();      // what bts_occupancy_eval_workspace returns
        char* ws = static_cast<char*>(malloc(bytes + off));
        Carver carve(ws + off);
        const OccEvalWs o = occ_eval_layout(carve, s[0], s[1], s[2]);
        bad += check("occ eval", carve, ws + off, ws + off + bytes, bytes, o.bins, o.sigma, (size_t)s[0] * 4, s);
        // the nested bins workspace holds lidar_bins_layout's carve wherever it starts
        Carver inner(o.bins);
        const LidarBins b = lidar_bins_layout(inner, s[1], s[2]);
        bad += reinterpret_cast<char*>(b.first) + (size_t)s[1] * s[2] * 8 > reinterpret_cast<char*>(o.tables);
        free(ws);
      }
      {
        Carver count(nullptr);
        bbox_eval_layout(count, s[0], s[1], s[2], s[3]);
        const size_t bytes = count.bytes();      // what bts_bbox_occupancy_eval_workspace returns
        char* ws = static_cast<char*>(malloc(bytes + off));
        Carver carve(ws + off);
        const BBoxEvalWs o = bbox_eval_layout(carve, s[0], s[1], s[2], s[3]);
        bad += check("bbox eval", carve, ws + off, ws + off + bytes, bytes, o.to_key, o.sigma, (size_t)s[0] * 4, s);
        free(ws);
      }
      {
        const int B = s[1], Hg = s[2], Wg = s[3];
        const size_t bytes = depth_metrics_bytes(B, Hg, Wg), nblk = (size_t)n_blocks(Hg, Wg);
        char* ws = static_cast<char*>(malloc(bytes + off));
        Carver carve(ws + off);
        DepthGeom g;
        depth_layout(carve, g, (size_t)B, nblk);
        bad += check("depth", carve, ws + off, ws + off + bytes, bytes, g.hist, g.mom, (size_t)B * nblk * kSlotDoubles * 8, s);
        free(ws);
      }
      {
        const int B = s[1], He = s[2], We = s[3];
        const size_t bytes = nvs_metrics_bytes(B, He, We);
        char* ws = static_cast<char*>(malloc(bytes + off));
        Carver carve(ws + off);
        NvsGeom g;
        nvs_layout(carve, g, (size_t)B, He, We);
        bad += check("nvs", carve, ws + off, ws + off + bytes, bytes, g.part, g.part,
                     (size_t)B * nvs_tiles(He, kTileY) * nvs_tiles(We, kTileX) * kNvsSlot * 8, s);
        free(ws);
      }
    }
  }
  printf(bad ? "FAILED\n" : "all layouts end where their size says\n");
  return bad ? 1 : 0;
}
