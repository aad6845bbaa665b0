// tetmesh.hip -- marching tetrahedra on the GPU: what utils/tetmesh.py:_unbatched_marching_tetrahedra computes with
// torch.unique(dim=0) on the six edges of every valid tetrahedron (moved to the CPU by mesh_extract_tetrahedra.py:96-97).
//
// Output vertex k is the k-th crossing edge (exactly one end with sdf > 0) in lexicographic (min, max) order; faces are
// every one-triangle tet in tet order, then every two-triangle tet in tet order (two consecutive triangles each).
// Restated as:
//   classify   -- per tet: triangle count (as a 1-or-2 packed pair for one 64-bit scan) and crossing-edge count;
//   scans      -- exclusive sums give each tet its first crossing-edge slot and its first face;
//   count read -- S (crossing-edge slots), n1, n2 to the host: the sort below needs S;
//   keys       -- one key (min << nb | max) per crossing-edge slot, nb = bits of N - 1, the slot as value;
//   sort       -- radix sort of the S keys over 2 nb bits only;
//   unique     -- head flags, inclusive scan -> vertex id per sorted slot; scattered back to the slots;
//   E read     -- the vertex count to the host (the caller sizes the outputs; torch.unique synchronises too);
//   emit       -- faces at their ordered offsets, endpoint positions / sdf / scales / ids per vertex.
// Only crossing edges enter the sort: a non-crossing edge of a valid tet never becomes a vertex, and every crossing
// edge belongs to a valid tet, so the vertex set and its order are those of the reference.
#include <hipcub/hipcub.hpp>

#include "common.h"

namespace ed3 {

namespace {

// utils/tetmesh.py:23-38, edge order (0,1),(0,2),(0,3),(1,2),(1,3),(2,3) (:40)
__constant__ int8_t c_tri_table[16][6] = {
    {-1, -1, -1, -1, -1, -1}, {1, 0, 2, -1, -1, -1}, {4, 0, 3, -1, -1, -1}, {1, 4, 2, 1, 3, 4},
    {3, 1, 5, -1, -1, -1},    {2, 3, 0, 2, 5, 3},    {1, 4, 0, 1, 5, 4},    {4, 2, 5, -1, -1, -1},
    {4, 5, 2, -1, -1, -1},    {4, 1, 0, 4, 5, 1},    {3, 2, 0, 3, 5, 2},    {1, 3, 5, -1, -1, -1},
    {4, 1, 2, 4, 3, 1},       {3, 0, 4, -1, -1, -1}, {2, 0, 1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1}};
__constant__ int8_t c_edge_a[6] = {0, 0, 0, 1, 1, 2};
__constant__ int8_t c_edge_b[6] = {1, 2, 3, 2, 3, 3};

struct TetWork {
    unsigned long long *code, *face_off;   // (is_one_triangle | is_two_triangles << 32), its exclusive sum
    uint32_t *cross, *cross_off;           // crossing edges per tet (0, 3 or 4), its exclusive sum
    unsigned long long *totals;            // S, n1, n2, bad-index count, E
    char *scan_temp;
    size_t scan_bytes;
};

struct EdgeWork {
    unsigned long long *keys, *keys_sorted, *ukey;
    uint32_t *slots, *slots_sorted, *flags, *vid, *slot_vid;
    char *temp;
    size_t temp_bytes;
};

size_t tet_scan_bytes(int T)
{
    size_t a = 0, b = 0;
    unsigned long long *u = nullptr;
    uint32_t *v = nullptr;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, u, u, T > 0 ? T : 1);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, v, v, T > 0 ? T : 1);
    return a > b ? a : b;
}

size_t edge_temp_bytes(int S)
{
    size_t a = 0, b = 0;
    unsigned long long *k = nullptr;
    uint32_t *v = nullptr;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, k, v, v, S > 0 ? S : 1, 0, 62);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, v, v, S > 0 ? S : 1);
    return a > b ? a : b;
}

size_t carve_tet(int T, char *base, TetWork *out)
{
    char *p = base;
    TetWork w;
    const size_t n = (size_t)(T > 0 ? T : 1);
    obtain(p, w.code, n);
    obtain(p, w.face_off, n);
    obtain(p, w.cross, n);
    obtain(p, w.cross_off, n);
    obtain(p, w.totals, 8);
    w.scan_bytes = tet_scan_bytes(T);
    obtain(p, w.scan_temp, w.scan_bytes);
    if (out) *out = w;
    return (size_t)(p - base) + 128;
}

size_t carve_edge(int S, char *base, EdgeWork *out)
{
    char *p = base;
    EdgeWork w;
    const size_t n = (size_t)(S > 0 ? S : 1);
    obtain(p, w.keys, n);
    obtain(p, w.keys_sorted, n);
    obtain(p, w.ukey, n);
    obtain(p, w.slots, n);
    obtain(p, w.slots_sorted, n);
    obtain(p, w.flags, n);
    obtain(p, w.vid, n);
    obtain(p, w.slot_vid, n);
    w.temp_bytes = edge_temp_bytes(S);
    obtain(p, w.temp, w.temp_bytes);
    if (out) *out = w;
    return (size_t)(p - base) + 128;
}

char *align128(const char *p) { return (char *)(((uintptr_t)p + 127) & ~(uintptr_t)127); }

// Occupancy bits of tet t; false (and bad += 1) when an index lies outside [0, N): such a tet is treated as outside
// everywhere, so no kernel below reads past `sdf` / `vertices`, and the host reports the error.
template <typename I>
__device__ inline bool load_tet(const I *__restrict__ tets, size_t t, int N, const float *__restrict__ sdf, int64_t v[4],
                                unsigned &occ)
{
    occ = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = (int64_t)tets[4 * t + k];
        if (v[k] < 0 || v[k] >= N) return false;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) occ |= (sdf[v[k]] > 0.f ? 1u : 0u) << k;   // NaN and 0 are outside (:100)
    return true;
}

template <typename I>
__global__ void __launch_bounds__(256) tet_classify_kernel(int T, int N, const I *__restrict__ tets,
                                                           const float *__restrict__ sdf, unsigned long long *__restrict__ code,
                                                           uint32_t *__restrict__ cross, unsigned long long *__restrict__ totals)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)T) return;
    int64_t v[4];
    unsigned occ;
    const bool in_range = load_tet(tets, t, N, sdf, v, occ);
    if (!in_range) atomicAdd(totals + 3, 1ull);
    const int n = __popc(occ);
    const bool valid = in_range && n > 0 && n < 4;
    code[t] = !valid ? 0ull : (n == 2 ? (1ull << 32) : 1ull);
    cross[t] = !valid ? 0u : (n == 2 ? 4u : 3u);
}

__global__ void tet_totals_kernel(int T, const unsigned long long *__restrict__ code, const unsigned long long *__restrict__ face_off,
                                  const uint32_t *__restrict__ cross, const uint32_t *__restrict__ cross_off,
                                  unsigned long long *__restrict__ totals)
{
    const unsigned long long f = face_off[T - 1] + code[T - 1];
    totals[0] = (unsigned long long)cross_off[T - 1] + cross[T - 1];
    totals[1] = f & 0xffffffffull;
    totals[2] = f >> 32;
}

template <typename I>
__global__ void __launch_bounds__(256) edge_keys_kernel(int T, int N, int nb, const I *__restrict__ tets,
                                                        const float *__restrict__ sdf, const uint32_t *__restrict__ cross,
                                                        const uint32_t *__restrict__ cross_off,
                                                        unsigned long long *__restrict__ keys, uint32_t *__restrict__ slots)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)T || cross[t] == 0) return;
    int64_t v[4];
    unsigned occ;
    load_tet(tets, t, N, sdf, v, occ);
    uint32_t slot = cross_off[t];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const int ea = c_edge_a[j], eb = c_edge_b[j];
        if (((occ >> ea) ^ (occ >> eb)) & 1u) {
            const uint64_t a = (uint64_t)min(v[ea], v[eb]), b = (uint64_t)max(v[ea], v[eb]);
            keys[slot] = (a << nb) | b;
            slots[slot] = slot;
            slot++;
        }
    }
}

__global__ void __launch_bounds__(256) edge_flags_kernel(int S, const unsigned long long *__restrict__ keys, uint32_t *__restrict__ flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) edge_scatter_kernel(int S, const unsigned long long *__restrict__ keys,
                                                           const uint32_t *__restrict__ slots, const uint32_t *__restrict__ flags,
                                                           const uint32_t *__restrict__ vid, uint32_t *__restrict__ slot_vid,
                                                           unsigned long long *__restrict__ ukey, unsigned long long *__restrict__ totals)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const uint32_t v = vid[i] - 1;
    slot_vid[slots[i]] = v;
    if (flags[i]) ukey[v] = keys[i];
    if (i == S - 1) totals[4] = vid[i];
}

template <typename I>
__global__ void __launch_bounds__(256) face_emit_kernel(int T, int N, const I *__restrict__ tets, const float *__restrict__ sdf,
                                                        const unsigned long long *__restrict__ code,
                                                        const unsigned long long *__restrict__ face_off,
                                                        const uint32_t *__restrict__ cross_off, long long n1,
                                                        const uint32_t *__restrict__ slot_vid, long long *__restrict__ faces)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)T || code[t] == 0) return;
    int64_t v[4];
    unsigned occ;
    load_tet(tets, t, N, sdf, v, occ);
    // slot of each of the six edges among the tet's crossing edges (edge order), -1 for non-crossing ones
    int rank[6];
    int r = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const bool c = ((occ >> c_edge_a[j]) ^ (occ >> c_edge_b[j])) & 1u;
        rank[j] = c ? r++ : -1;
    }
    const bool two = code[t] >> 32;
    const unsigned long long fo = face_off[t];
    const long long f0 = two ? n1 + 2 * (long long)(fo >> 32) : (long long)(fo & 0xffffffffull);
    const uint32_t base = cross_off[t];
    const int nc = two ? 6 : 3;
    for (int k = 0; k < nc; k++) {
        const int e = c_tri_table[occ][k];
        int rk = 0;
#pragma unroll
        for (int j = 0; j < 6; j++) if (j == e) rk = rank[j];
        faces[3 * f0 + k] = (long long)slot_vid[base + rk];
    }
}

__global__ void __launch_bounds__(256) vertex_emit_kernel(int E, int nb, const unsigned long long *__restrict__ ukey,
                                                          const float *__restrict__ vertices, const float *__restrict__ sdf,
                                                          const float *__restrict__ scales, float *__restrict__ out_verts,
                                                          float *__restrict__ out_sdf, float *__restrict__ out_scales,
                                                          long long *__restrict__ out_ids)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= E) return;
    const unsigned long long k = ukey[v];
    const long long ab[2] = {(long long)(k >> nb), (long long)(k & ((1ull << nb) - 1))};
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const size_t o = 2 * (size_t)v + e;
        out_verts[3 * o + 0] = vertices[3 * ab[e] + 0];
        out_verts[3 * o + 1] = vertices[3 * ab[e] + 1];
        out_verts[3 * o + 2] = vertices[3 * ab[e] + 2];
        out_sdf[o] = sdf[ab[e]];
        out_scales[o] = scales[ab[e]];
        out_ids[o] = ab[e];
    }
}

int index_bits(int N) { int nb = 1; while (nb < 31 && (1ll << nb) < (long long)N) nb++; return nb; }

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

}  // namespace ed3

using namespace ed3;

extern "C" {

size_t ed3dgs_tetmesh_tet_bytes(int T) { return carve_tet(T, nullptr, nullptr); }
size_t ed3dgs_tetmesh_edge_bytes(int S) { return carve_edge(S, nullptr, nullptr); }

int ed3dgs_tetmesh_count(int N, int T, const void *tets, int tets_int64, const float *sdf, char *tet_ws, size_t tet_ws_bytes,
                         ed3dgs_alloc_fn edge_alloc, void *edge_user, long long counts[4], void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (N < 0 || T < 0 || T > (1 << 29) || !counts || !edge_alloc) { set_error("ed3dgs_tetmesh_count: bad N/T or null counts/allocator"); return ED3DGS_ERR_INVALID; }
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (T == 0) return 0;
    if (!tets || !sdf || !tet_ws || tet_ws_bytes < ed3dgs_tetmesh_tet_bytes(T)) { set_error("ed3dgs_tetmesh_count: null pointer or workspace too small"); return ED3DGS_ERR_INVALID; }
    TetWork w;
    carve_tet(T, align128(tet_ws), &w);
    if (!check_hip(hipMemsetAsync(w.totals, 0, 8 * sizeof(unsigned long long), s), "tetmesh: memset totals")) return ED3DGS_ERR_HIP;
    if (tets_int64)
        hipLaunchKernelGGL(tet_classify_kernel<int64_t>, dim3(blocks(T)), dim3(256), 0, s, T, N, (const int64_t *)tets, sdf, w.code, w.cross, w.totals);
    else
        hipLaunchKernelGGL(tet_classify_kernel<int32_t>, dim3(blocks(T)), dim3(256), 0, s, T, N, (const int32_t *)tets, sdf, w.code, w.cross, w.totals);
    size_t b = w.scan_bytes;
    if (!check_hip(hipcub::DeviceScan::ExclusiveSum(w.scan_temp, b, w.code, w.face_off, T, s), "tetmesh: face scan")) return ED3DGS_ERR_HIP;
    b = w.scan_bytes;
    if (!check_hip(hipcub::DeviceScan::ExclusiveSum(w.scan_temp, b, w.cross, w.cross_off, T, s), "tetmesh: edge scan")) return ED3DGS_ERR_HIP;
    hipLaunchKernelGGL(tet_totals_kernel, dim3(1), dim3(1), 0, s, T, w.code, w.face_off, w.cross, w.cross_off, w.totals);
    unsigned long long tot[8];
    if (!check_hip(hipMemcpyAsync(tot, w.totals, sizeof(tot), hipMemcpyDeviceToHost, s), "tetmesh: count read") ||
        !check_hip(hipStreamSynchronize(s), "tetmesh: classify")) return ED3DGS_ERR_HIP;
    if (tot[3]) { set_error("ed3dgs_tetmesh_count: " + std::to_string(tot[3]) + " tets hold a vertex index outside [0, N)"); return ED3DGS_ERR_INVALID; }
    if (tot[0] > 0x7fffffffull) { set_error("ed3dgs_tetmesh_count: more than 2^31 - 1 crossing-edge slots"); return ED3DGS_ERR_INVALID; }
    const int S = (int)tot[0];
    counts[1] = (long long)tot[1];
    counts[2] = (long long)tot[2];
    counts[3] = S;
    char *ec = edge_alloc(edge_user, ed3dgs_tetmesh_edge_bytes(S));
    if (!ec) { set_error("tetmesh: edge workspace allocation failed"); return ED3DGS_ERR_ALLOC; }
    if (S == 0) return 0;
    EdgeWork e;
    carve_edge(S, align128(ec), &e);
    const int nb = index_bits(N);
    if (tets_int64)
        hipLaunchKernelGGL(edge_keys_kernel<int64_t>, dim3(blocks(T)), dim3(256), 0, s, T, N, nb, (const int64_t *)tets, sdf, w.cross, w.cross_off, e.keys, e.slots);
    else
        hipLaunchKernelGGL(edge_keys_kernel<int32_t>, dim3(blocks(T)), dim3(256), 0, s, T, N, nb, (const int32_t *)tets, sdf, w.cross, w.cross_off, e.keys, e.slots);
    b = e.temp_bytes;
    if (!check_hip(hipcub::DeviceRadixSort::SortPairs(e.temp, b, e.keys, e.keys_sorted, e.slots, e.slots_sorted, S, 0, 2 * nb, s),
                   "tetmesh: edge sort")) return ED3DGS_ERR_HIP;
    hipLaunchKernelGGL(edge_flags_kernel, dim3(blocks(S)), dim3(256), 0, s, S, e.keys_sorted, e.flags);
    b = e.temp_bytes;
    if (!check_hip(hipcub::DeviceScan::InclusiveSum(e.temp, b, e.flags, e.vid, S, s), "tetmesh: unique scan")) return ED3DGS_ERR_HIP;
    hipLaunchKernelGGL(edge_scatter_kernel, dim3(blocks(S)), dim3(256), 0, s, S, e.keys_sorted, e.slots_sorted, e.flags, e.vid,
                       e.slot_vid, e.ukey, w.totals);
    if (!check_hip(hipMemcpyAsync(tot, w.totals, sizeof(tot), hipMemcpyDeviceToHost, s), "tetmesh: vertex count read") ||
        !check_hip(hipStreamSynchronize(s), "tetmesh: unique")) return ED3DGS_ERR_HIP;
    counts[0] = (long long)tot[4];
    return 0;
}

int ed3dgs_tetmesh_emit(int N, int T, const void *tets, int tets_int64, const float *vertices, const float *sdf,
                        const float *scales, const char *tet_ws, const char *edge_ws, const long long counts[4],
                        float *out_verts, float *out_sdf, float *out_scales, long long *out_faces, long long *out_ids,
                        void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (!counts) { set_error("ed3dgs_tetmesh_emit: null counts"); return ED3DGS_ERR_INVALID; }
    const long long E = counts[0], n1 = counts[1], n2 = counts[2], S = counts[3];
    if (S == 0) return 0;
    if (!tets || !vertices || !sdf || !scales || !tet_ws || !edge_ws || !out_verts || !out_sdf || !out_scales || !out_faces || !out_ids) {
        set_error("ed3dgs_tetmesh_emit: null pointer"); return ED3DGS_ERR_INVALID;
    }
    TetWork w;
    EdgeWork e;
    carve_tet(T, align128(tet_ws), &w);
    carve_edge((int)S, align128(edge_ws), &e);
    (void)n2;
    if (tets_int64)
        hipLaunchKernelGGL(face_emit_kernel<int64_t>, dim3(blocks(T)), dim3(256), 0, s, T, N, (const int64_t *)tets, sdf, w.code,
                           w.face_off, w.cross_off, n1, e.slot_vid, out_faces);
    else
        hipLaunchKernelGGL(face_emit_kernel<int32_t>, dim3(blocks(T)), dim3(256), 0, s, T, N, (const int32_t *)tets, sdf, w.code,
                           w.face_off, w.cross_off, n1, e.slot_vid, out_faces);
    if (E > 0)
        hipLaunchKernelGGL(vertex_emit_kernel, dim3(blocks((size_t)E)), dim3(256), 0, s, (int)E, index_bits(N), e.ukey, vertices,
                           sdf, scales, out_verts, out_sdf, out_scales, out_ids);
    return check_hip(hipGetLastError(), "tetmesh emit") ? 0 : ED3DGS_ERR_HIP;
}

}  // extern "C"
