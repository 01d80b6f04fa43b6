// The ground-truth half of the 3D-bounding-box occupancy evaluator (models/bts/evaluator_3dbb.py:30-60, 63-74, 102-128, 146-150,
// 236-241, 257-299) as three short fp32 kernels: one table of face normals and slab bounds per box, the pseudo depth of every ray
// (the z of its nearest valid slab intercept among the boxes that carry the ray's label), and the classification of the query points
// into the six counters of occ_metrics_kernel.  No matrix pipe, no inline assembly; the only reductions are an int32 add and a
// bit-pattern minimum of positive floats, so reruns are bit-identical.
#include "bts_host.h"
#include "bts_eval_device.h"

namespace bts {

constexpr int kFaces = BTS_BBOX_MAX_FACES;    // rows of a box's table
constexpr int kVerts = BTS_BBOX_MAX_VERTS;
constexpr int kBoxesPerLaunch = 256;          // offsets travel as kernel arguments, this many boxes at a time
constexpr int kChunk = 16;                    // boxes staged in LDS at a time (16 * 32 * 7 floats = 14 KB)
constexpr int kRow = 7;                       // a staged face: nx ny nz lo hi (lo - EPS) (hi + EPS)
constexpr float kSlabEps = 1e-4f;             // EPS, evaluator_3dbb.py:25
constexpr unsigned kPosInfBits = 0x7F800000u;

struct BBoxOffsets {
  int v[kBoxesPerLaunch + 1], f[kBoxesPerLaunch + 1];
};

// verts_to_cam (:30-35), bbox_in_frustum (:38-44), compute_bounds (:47-60).  One wave per box: lane = vertex, then lane = face.
// tables (B, 32, 5): (nx, ny, nz, lo, hi) per face, zeros in the unused rows.  A degenerate face divides 0 by 0: its row is NaN and
// stays NaN.  A face index outside the box's vertices is clamped into them (nothing faults; the row is unspecified).
__global__ __launch_bounds__(64) void bbox_bounds_kernel(const float* __restrict__ vertices, const int* __restrict__ faces, BBoxOffsets offs, int box0,
                                                         const float* __restrict__ to_key, const float* __restrict__ proj, float max_d,
                                                         float* __restrict__ tables, int* __restrict__ n_faces, unsigned char* __restrict__ active,
                                                         int* __restrict__ n_active) {
  __shared__ float s_v[kVerts * 3];
  const int k = blockIdx.x, lane = threadIdx.x;
  const int v0 = offs.v[k], V = offs.v[k + 1] - v0;
  const int f0 = offs.f[k], F = offs.f[k + 1] - f0;
  const long b = (long)box0 + k;
  bool in = false;
  if (lane < V) {
    const float* p = vertices + ((long)v0 + lane) * 3;
    const float x = p[0], y = p[1], z = p[2];
    // pose[:3, :3] @ verts.T + pose[:3, 3, None] (:32)
    const float cx = ((to_key[0] * x + to_key[1] * y) + to_key[2] * z) + to_key[3];
    const float cy = ((to_key[4] * x + to_key[5] * y) + to_key[6] * z) + to_key[7];
    const float cz = ((to_key[8] * x + to_key[9] * y) + to_key[10] * z) + to_key[11];
    s_v[lane * 3 + 0] = cx, s_v[lane * 3 + 1] = cy, s_v[lane * 3 + 2] = cz;
    // projs @ verts.T, x and y over z (:40-42)
    const float uz = (proj[6] * cx + proj[7] * cy) + proj[8] * cz;
    const float ux = ((proj[0] * cx + proj[1] * cy) + proj[2] * cz) / uz;
    const float uy = ((proj[3] * cx + proj[4] * cy) + proj[5] * cz) / uz;
    in = ((ux >= -1.0f) & (ux <= 1.0f)) & ((uy >= -1.0f) & (uy <= 1.0f)) & ((uz > 0.0f) & (uz <= max_d));
  }
  const bool act = __ballot(in) != 0ull;   // reducer = torch.any (:216)
  __syncthreads();
  if (lane < kFaces) {
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, lo = 0.0f, hi = 0.0f;
    if (lane < F) {
      const int* f = faces + ((long)f0 + lane) * 3;
      const int i0 = min(max(f[0], 0), V - 1), i1 = min(max(f[1], 0), V - 1), i2 = min(max(f[2], 0), V - 1);
      const float ax = s_v[i1 * 3 + 0] - s_v[i0 * 3 + 0], ay = s_v[i1 * 3 + 1] - s_v[i0 * 3 + 1], az = s_v[i1 * 3 + 2] - s_v[i0 * 3 + 2];
      const float bx = s_v[i2 * 3 + 0] - s_v[i0 * 3 + 0], by = s_v[i2 * 3 + 1] - s_v[i0 * 3 + 1], bz = s_v[i2 * 3 + 2] - s_v[i0 * 3 + 2];
      // torch.cross, then the division by torch.norm (:52-54)
      const float kx = ay * bz - az * by, ky = az * bx - ax * bz, kz = ax * by - ay * bx;
      const float len = sqrtf((kx * kx + ky * ky) + kz * kz);
      nx = kx / len, ny = ky / len, nz = kz / len;
      // min and max of face_normals @ vertices.T (:56-58)
      lo = hi = (nx * s_v[0] + ny * s_v[1]) + nz * s_v[2];
      for (int v = 1; v < V; ++v) {
        const float pr = (nx * s_v[v * 3 + 0] + ny * s_v[v * 3 + 1]) + nz * s_v[v * 3 + 2];
        lo = fminf(lo, pr), hi = fmaxf(hi, pr);
      }
    }
    float* row = tables + (b * kFaces + lane) * 5;
    row[0] = nx, row[1] = ny, row[2] = nz, row[3] = lo, row[4] = hi;
  }
  if (lane == 0) {
    n_faces[b] = F;
    active[b] = act ? 1 : 0;
    if (act && n_active) atomicAdd(n_active, 1);
  }
}

// the tables of the boxes [c0, c0 + nb) into LDS, with the two widened bounds of in_bbox (:70) formed once
__device__ __forceinline__ void stage_boxes(const float* __restrict__ tables, const int* __restrict__ n_faces, const unsigned char* __restrict__ active,
                                            const float* __restrict__ semantic_id, int c0, int nb, float* s_tab, int* s_nf, float* s_sem) {
  for (int i = threadIdx.x; i < nb * kFaces; i += 256) {
    const float* src = tables + ((long)c0 * kFaces + i) * 5;
    float* dst = s_tab + i * kRow;
    const float lo = src[3], hi = src[4];
    dst[0] = src[0], dst[1] = src[1], dst[2] = src[2], dst[3] = lo, dst[4] = hi;
    dst[5] = lo - kSlabEps, dst[6] = hi + kSlabEps;
  }
  if (threadIdx.x < nb) {
    s_nf[threadIdx.x] = active[c0 + threadIdx.x] ? min(max(n_faces[c0 + threadIdx.x], 0), kFaces) : 0;   // an inactive box: no faces to walk
    if (semantic_id) s_sem[threadIdx.x] = semantic_id[c0 + threadIdx.x];
  }
}

// in_bbox (:63-74) of one point against one staged box: every slab comparison must hold (a NaN row holds none)
__device__ __forceinline__ bool in_staged_box(const float* T, int m, float px, float py, float pz) {
  for (int i = 0; i < m; ++i) {
    const float pr = (T[i * kRow + 0] * px + T[i * kRow + 1] * py) + T[i * kRow + 2] * pz;
    if (!((T[i * kRow + 5] <= pr) & (pr <= T[i * kRow + 6]))) return false;
  }
  return true;
}

// bbox_intercept_labeled (:102-128) over the boxes and the argmin over boxes (:236-241), of which only z survives.  lane = ray,
// blockIdx.y = a chunk of kChunk boxes; out (R): the bit pattern of the smallest valid p_z (p_z > 0, so the uint32 order is the float
// order), preset to +inf by the launcher.
__global__ __launch_bounds__(256) void bbox_pseudo_depth_kernel(const float* __restrict__ rays, int R, int pw, const float* __restrict__ seg, int hs,
                                                                int ws, float sh, float sw, const float* __restrict__ tables,
                                                                const int* __restrict__ n_faces, const unsigned char* __restrict__ active,
                                                                const float* __restrict__ semantic_id, int B, unsigned* __restrict__ out) {
  __shared__ float s_tab[kChunk * kFaces * kRow];
  __shared__ int s_nf[kChunk];
  __shared__ float s_sem[kChunk];
  const int c0 = blockIdx.y * kChunk;
  const int nb = min(kChunk, B - c0);
  stage_boxes(tables, n_faces, active, semantic_id, c0, nb, s_tab, s_nf, s_sem);
  __syncthreads();
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const int y = r / pw, x = r - y * pw;
  // the label of F.interpolate(seg, (ph, pw), mode="nearest") at the ray's pixel (:231)
  const float label = seg[(long)nearest_src(y, sh, hs) * ws + nearest_src(x, sw, ws)];
  const float dx = rays[(long)r * 8 + 3], dy = rays[(long)r * 8 + 4], dz = rays[(long)r * 8 + 5];
  float best = __uint_as_float(kPosInfBits);
  for (int box = 0; box < nb; ++box) {
    const int m = s_nf[box];
    if (m == 0 || !(s_sem[box] == label)) continue;
    const float* T = s_tab + box * kFaces * kRow;
    for (int j = 0; j < m; ++j) {
      const float denom = (T[j * kRow + 0] * dx + T[j * kRow + 1] * dy) + T[j * kRow + 2] * dz;
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const float t = T[j * kRow + 3 + side] / denom;
        const float px = t * dx, py = t * dy, pz = t * dz;
        // p_z > 0 (:119); a candidate at or beyond the best so far cannot lower the minimum
        if (!(pz > 0.0f) || !(pz < best)) continue;
        if (in_staged_box(T, m, px, py, pz)) best = pz;
      }
    }
  }
  if (best < __uint_as_float(kPosInfBits)) atomicMin(&out[r], __float_as_uint(best));
}

// BTSWrapper.forward :257-299 per query point (key frame): project_into_cam (:146-150), the nearest look-up in the pseudo depth and in
// the predicted z-depth (:259-260), V = dist <= gt | dist <= pred (:261), O = in_bbox of any active box & !V (:264-275),
// P = sigma > threshold (:286), and the cell of (V, O, P) in bts_eval_device.h's order, counted by its count_cells.  masks (3, P): P, O, V
// as bytes, when given.
__global__ __launch_bounds__(256) void bbox_metrics_kernel(const float* __restrict__ q_pts, int P, const float* __restrict__ sigma,
                                                           const float* __restrict__ pseudo, const float* __restrict__ depth_z, int H, int W,
                                                           const float* __restrict__ proj, const float* __restrict__ tables,
                                                           const int* __restrict__ n_faces, const unsigned char* __restrict__ active, int B,
                                                           float occ_threshold, int* __restrict__ counts, unsigned char* __restrict__ masks) {
  __shared__ float s_tab[kChunk * kFaces * kRow];
  __shared__ int s_nf[kChunk];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < P;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (valid) px = q_pts[(long)i * 3 + 0], py = q_pts[(long)i * 3 + 1], pz = q_pts[(long)i * 3 + 2];
  bool inside = false;
  for (int c0 = 0; c0 < B; c0 += kChunk) {
    const int nb = min(kChunk, B - c0);
    __syncthreads();
    stage_boxes(tables, n_faces, active, nullptr, c0, nb, s_tab, s_nf, nullptr);
    __syncthreads();
    if (valid && !inside)
      for (int box = 0; box < nb && !inside; ++box)
        if (s_nf[box] > 0) inside = in_staged_box(s_tab + box * kFaces * kRow, s_nf[box], px, py, pz);
  }
  int cell = -1;
  if (valid) {
    const float ux = (proj[0] * px + proj[1] * py) + proj[2] * pz;
    const float uy = (proj[3] * px + proj[4] * py) + proj[5] * pz;
    const float dist = (proj[6] * px + proj[7] * py) + proj[8] * pz;
    const long texel = nearest_border_texel(ux / dist, uy / dist, H, W);
    const bool V = (dist <= pseudo[texel]) | (dist <= depth_z[texel]);   // a ray no box stops has +inf pseudo depth: visible
    const bool O = inside & !V;
    const bool Pm = sigma[i] > occ_threshold;
    // the twin of occ_metrics_kernel's lines (bts_occ.hip): as a function of bts_eval_device.h they change both kernels' instructions
    cell = V ? (Pm ? 0 : 1) : (O ? (Pm ? 2 : 3) : (Pm ? 4 : 5));
    if (masks) {
      masks[i] = Pm ? 1 : 0;
      masks[(long)P + i] = O ? 1 : 0;
      masks[2L * P + i] = V ? 1 : 0;
    }
  }
  count_cells(cell, counts);
}

// THE layout of bts_bbox_occupancy_eval's workspace.  tables, pseudo and sigma keep their slots when the caller brings buffers of its own
BBoxEvalWs bbox_eval_layout(Carver& w, int P, int B, int ph, int pw) {
  BBoxEvalWs o;
  o.to_key = w.take<float>(16);
  o.tables = w.take<float>((size_t)B * kFaces * 5);
  o.n_faces = w.take<int>((size_t)B);
  o.active = w.take<unsigned char>((size_t)B);
  o.pseudo = w.take<float>((size_t)ph * pw);
  o.sigma = w.take<float>((size_t)P);
  return o;
}

// v_offsets, f_offsets: HOST arrays of B + 1 entries (validated by the caller).  n_active: one int32 the active boxes are ADDED to, or NULL
int bbox_bounds_launch(const float* vertices, const int* faces, const int* v_offsets, const int* f_offsets, int B, const float* to_key,
                       const float* proj, float max_d, float* tables, int* n_faces, unsigned char* active, int* n_active, hipStream_t s) {
  for (int box0 = 0; box0 < B; box0 += kBoxesPerLaunch) {
    const int nb = B - box0 < kBoxesPerLaunch ? B - box0 : kBoxesPerLaunch;
    BBoxOffsets offs;
    for (int k = 0; k <= nb; ++k) offs.v[k] = v_offsets[box0 + k], offs.f[k] = f_offsets[box0 + k];
    bbox_bounds_kernel<<<nb, 64, 0, s>>>(vertices, faces, offs, box0, to_key, proj, max_d, tables, n_faces, active, n_active);
    if (int rc = launch_code()) return rc;
  }
  return BTS_OK;
}

int bbox_pseudo_depth_launch(const float* rays, int ph, int pw, const float* seg, int hs, int ws, const float* tables, const int* n_faces,
                             const unsigned char* active, const float* semantic_id, int B, float* pseudo_depth, hipStream_t s) {
  const int R = ph * pw;
  if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(pseudo_depth), (int)kPosInfBits, (size_t)R, s) != hipSuccess) {
    (void)launch_code();
    return BTS_E_LAUNCH;
  }
  const float sh = (float)hs / (float)ph, sw = (float)ws / (float)pw;
  bbox_pseudo_depth_kernel<<<dim3((R + 255) / 256, (B + kChunk - 1) / kChunk), 256, 0, s>>>(rays, R, pw, seg, hs, ws, sh, sw, tables, n_faces, active,
                                                                                           semantic_id, B, reinterpret_cast<unsigned*>(pseudo_depth));
  return launch_code();
}

// counts: the six cells, ADDED to (the caller zeroes them)
int bbox_metrics_launch(const float* q_pts, int P, const float* sigma, const float* pseudo, const float* depth_z, int H, int W, const float* proj,
                        const float* tables, const int* n_faces, const unsigned char* active, int B, float occ_threshold, int* counts,
                        unsigned char* masks, hipStream_t s) {
  bbox_metrics_kernel<<<(P + 255) / 256, 256, 0, s>>>(q_pts, P, sigma, pseudo, depth_z, H, W, proj, tables, n_faces, active, B, occ_threshold, counts,
                                                     masks);
  return launch_code();
}

}  // namespace bts
