// Pose-graph optimisation over Sim(3) (include/vslam_graph.h): a batch of independent graphs, one workgroup of 256 lanes per graph
// and ONE launch; every decision and every expression is graph_math.h's gr_run, which tests/native/graph_serial.cpp walks on the
// host.  This file adds what knows about lanes: who owns which unit (lane l takes units l, l + 256, ... of every pass, nodes and
// edges alike, so a node's vectors stay with one lane between barriers), the sums (per-lane partial sums closed by
// block_reduce.h: no floating-point atomics), and the adjacency (integer counts, block_scan.h, and a fill that ranks the edges of a
// chunk of 256 against each other in LDS, so a node's list is in ascending edge index whatever the lanes' timing).
// The CG vectors, the blocks and the edges' linearisations live in the arena, i.e. in L2 (DESIGN.md 5o says why); LDS holds the
// reduction's four words, the scan's four and the fill's two columns.
#include <algorithm>
#include <cmath>

#include "block_reduce.h"
#include "block_scan.h"
#include "ctx.h"
#include "graph_math.h"
#include "../../include/vslam_graph.h"

#pragma clang fp contract(off)

using namespace vs_graph;

namespace {
constexpr int kGT = 256;   // lanes per workgroup

struct GraphArgs {
    double *scale, *R, *T;
    const int32_t *fixed, *ab, *n_nodes, *n_edges;
    const double *z_scale, *z_R, *z_T, *z_w;
    int node_stride, edge_stride;
    unsigned char *workspace;
    size_t workspace_item;
    double *stats;
    GrParams prm;
};

struct GrBlock {
    VsBlockReduce rd;
    int *scan, *col_a, *col_b;

    template <class F>
    __device__ __forceinline__ void each(int n, F f) const {
        for (int i = threadIdx.x; i < n; i += kGT) f(i);
    }
    template <int N>
    __device__ __forceinline__ void sum(double (&v)[N]) const {
        rd.sum(v);
    }
    __device__ __forceinline__ bool any(bool f) const { return rd.any(f); }
    __device__ __forceinline__ void sync() const { __syncthreads(); }

    // start [N + 1] and adj from use: counts, a scan, a stable fill
    __device__ __forceinline__ void adjacency(const GrItem &it, int N, int E) const {
        const int tid = threadIdx.x;
        for (int i = tid; i < N; i += kGT) it.fill[i] = 0;
        __syncthreads();
        for (int k = tid; k < E; k += kGT) {
            if (!it.use[k]) continue;
            atomicAdd(&it.fill[it.ab[2 * (size_t)k]], 1);       // integers: the count is the same in any order
            atomicAdd(&it.fill[it.ab[2 * (size_t)k + 1]], 1);
        }
        __syncthreads();
        int running = 0;   // the same in every lane
        for (int base = 0; base < N; base += kGT) {
            const int i = base + tid;
            const int v = i < N ? it.fill[i] : 0;
            int total;
            const int before = vs_block_excl_scan<kGT>(v, scan, total);
            if (i < N) it.start[i] = running + before;
            running += total;
        }
        if (tid == 0) it.start[N] = running;
        __syncthreads();
        for (int i = tid; i < N; i += kGT) it.fill[i] = 0;
        __syncthreads();
        for (int base = 0; base < E; base += kGT) {
            const int k = base + tid;
            int a = -1, b = -1;
            if (k < E && it.use[k]) {
                a = it.ab[2 * (size_t)k];
                b = it.ab[2 * (size_t)k + 1];
            }
            col_a[tid] = a;
            col_b[tid] = b;
            __syncthreads();
            if (a >= 0) {
                int ra = 0, rb = 0;   // the earlier edges of this chunk at each of the two nodes
                for (int j = 0; j < tid; j++) {
                    const int ja = col_a[j], jb = col_b[j];
                    ra += (ja == a ? 1 : 0) + (jb == a ? 1 : 0);
                    rb += (ja == b ? 1 : 0) + (jb == b ? 1 : 0);
                }
                it.adj[it.start[a] + it.fill[a] + ra] = k << 1;
                it.adj[it.start[b] + it.fill[b] + rb] = (k << 1) | 1;
            }
            __syncthreads();   // fill has been read by everyone
            if (a >= 0) {
                atomicAdd(&it.fill[a], 1);
                atomicAdd(&it.fill[b], 1);
            }
            __syncthreads();
        }
    }
};

__global__ __launch_bounds__(kGT) void graph_optimize_kernel(GraphArgs a) {
    __shared__ double red[kGT / 64];
    __shared__ int scan[kGT / 64];
    __shared__ int col_a[kGT], col_b[kGT];
    const int b = blockIdx.x;
    const size_t Ns = (size_t)a.node_stride, Es = (size_t)a.edge_stride;
    GrItem it;
    it.n_nodes = a.n_nodes[b];
    it.n_edges = a.n_edges[b];
    it.node_stride = a.node_stride;
    it.edge_stride = a.edge_stride;
    it.scale = a.scale + b * Ns;
    it.R = a.R + b * Ns * 9;
    it.T = a.T + b * Ns * 3;
    it.fixed = a.fixed + b * Ns;
    it.ab = a.ab + b * Es * 2;
    it.z_scale = a.z_scale + b * Es;
    it.z_R = a.z_R + b * Es * 9;
    it.z_T = a.z_T + b * Es * 3;
    it.z_w = a.z_w + b * Es * 3;
    gr_workspace(a.workspace + b * a.workspace_item, it);
    GrBlock par{VsBlockReduce{red}, scan, col_a, col_b};
    double stats[4];
    int cg_total;
    gr_run(par, it, a.prm, stats, cg_total);
    if (a.stats && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) a.stats[(size_t)b * 4 + k] = stats[k];
    }
}

// ---- on the world
struct LoopList {
    const int32_t *__restrict__ track, *__restrict__ frame_a, *__restrict__ frame_b, *__restrict__ use;
    const double *__restrict__ scale, *__restrict__ R, *__restrict__ T;
    int loops;
};

struct WorldGraph {
    int max_frames, frames, edge_stride;
    double w_seq[3], w_loop[3];
    // the graph of each track, [tracks] x ...
    double *scale, *R, *T, *prev_R, *prev_T;           // [frames], [frames][9], [frames][3]; prev: W and C as the call found them
    int32_t *fixed, *n_nodes, *n_edges, *ab;           // [frames], 1, 1, [edge_stride][2]
    double *z_scale, *z_R, *z_T, *z_w;                 // [edge_stride] ...
};

// one workgroup per track: nodes from d_Twc, the sequential edges, then the taken loops of the track compacted in list order
__global__ __launch_bounds__(kGT) void graph_world_gather_kernel(WorldGraph g, LoopList l, int tracks, const double *__restrict__ Twc) {
    __shared__ int wave_n[kGT / 64];
    const int t = blockIdx.x, tid = threadIdx.x, F = g.frames;
    const size_t n0 = (size_t)t * F, e0 = (size_t)t * g.edge_stride;
    const double *pose = Twc + (size_t)t * g.max_frames * 16;
    for (int f = tid; f < F; f += kGT) {
        const double *P = pose + (size_t)f * 16;
        g.scale[n0 + f] = 1.0;
        g.fixed[n0 + f] = f == 0 ? 1 : 0;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) g.R[(n0 + f) * 9 + 3 * r + c] = g.prev_R[(n0 + f) * 9 + 3 * r + c] = P[4 * r + c];
            g.T[(n0 + f) * 3 + r] = g.prev_T[(n0 + f) * 3 + r] = P[4 * r + 3];
        }
        if (f + 1 >= F) continue;
        const double *Q = P + 16;   // frame f + 1: W', C'
        const size_t e = e0 + f;
        g.ab[2 * e] = f;
        g.ab[2 * e + 1] = f + 1;
        g.z_scale[e] = 1.0;
        const double c[3] = {P[3] - Q[3], P[7] - Q[7], P[11] - Q[11]};
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) g.z_R[e * 9 + 3 * i + j] = (Q[i] * P[j] + Q[4 + i] * P[4 + j]) + Q[8 + i] * P[8 + j];
            g.z_T[e * 3 + i] = (Q[i] * c[0] + Q[4 + i] * c[1]) + Q[8 + i] * c[2];
            g.z_w[e * 3 + i] = g.w_seq[i];
        }
    }
    const int room = g.edge_stride - (F - 1);
    int running = 0;   // the same in every lane
    for (int base = 0; base < l.loops; base += kGT) {
        const int k = base + tid;
        bool take = false;
        GrNodeV Z;
        int fa = 0, fb = 0;
        if (k < l.loops && l.use[k] != 0 && l.track[k] == t) {
            fa = l.frame_a[k];
            fb = l.frame_b[k];
            Z.s = l.scale[k];
#pragma unroll
            for (int j = 0; j < 9; j++) Z.R[j] = l.R[(size_t)k * 9 + j];
#pragma unroll
            for (int j = 0; j < 3; j++) Z.t[j] = l.T[(size_t)k * 3 + j];
            take = fa != fb && fa >= 0 && fa < F && fb >= 0 && fb < F && gr_finite(Z) && Z.s > 0.0;
        }
        int total;
        const int slot = running + vs_block_flag_scan<kGT>(take, wave_n, total);
        running += total;
        if (!take || slot >= room) continue;
        const size_t e = e0 + (F - 1) + slot;
        g.ab[2 * e] = fa;
        g.ab[2 * e + 1] = fb;
        g.z_scale[e] = Z.s;
#pragma unroll
        for (int j = 0; j < 9; j++) g.z_R[e * 9 + j] = Z.R[j];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            g.z_T[e * 3 + j] = Z.t[j];
            g.z_w[e * 3 + j] = g.w_loop[j];
        }
    }
    if (tid == 0) {
        g.n_nodes[t] = F;
        g.n_edges[t] = running > 0 ? (F - 1) + min(running, room) : 0;   // no taken loop: no edge, the track is left alone
    }
}

// one workgroup per track, behind the optimisation: where it moved, frames 1 .. F - 1 (node 0 is held, every other node has its
// sequential edge) into the world's arrays, the carry, and every point with its anchor
__global__ __launch_bounds__(kGT) void graph_world_scatter_kernel(WorldGraph g, const double *__restrict__ stats, double *__restrict__ stats_out,
                                                                  int kp_stride, int map_capacity, int obs_capacity,
                                                                  const int32_t *__restrict__ sizes, const int32_t *__restrict__ off,
                                                                  const int32_t *__restrict__ obs_frame, double *Twc, float *pose, double *scale,
                                                                  double *carry, const int32_t *__restrict__ carry_idx, float4 *points) {
    const int t = blockIdx.x, tid = threadIdx.x, F = g.frames;
    const size_t n0 = (size_t)t * F;
    if (stats_out && tid < 4) stats_out[(size_t)t * 4 + tid] = stats[(size_t)t * 4 + tid];
    const double accepted = stats[(size_t)t * 4 + 3];
    if (!(accepted == accepted)) return;   // NaN: the track was left alone
    for (int f = 1 + tid; f < F; f += kGT) {
        const size_t fr = (size_t)t * g.max_frames + f;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) Twc[fr * 16 + 4 * r + c] = g.R[(n0 + f) * 9 + 3 * r + c];
            Twc[fr * 16 + 4 * r + 3] = g.T[(n0 + f) * 3 + r];
        }
#pragma unroll
        for (int k = 0; k < 16; k++) pose[fr * 16 + k] = (float)Twc[fr * 16 + k];
        scale[fr] = scale[fr] * g.scale[n0 + f];
    }
    if (F > 1) {
        const double s = g.scale[n0 + F - 1];
        for (int k = tid; k < kp_stride; k += kGT) {
            const size_t r = (size_t)t * kp_stride + k;
            if (carry_idx[r] < 0) continue;
#pragma unroll
            for (int c = 0; c < 3; c++) carry[3 * r + c] = carry[3 * r + c] * s;
        }
    }
    const int n = min(max(sizes[t], 0), map_capacity);
    const int32_t *o = off + (size_t)t * (map_capacity + 1);
    for (int i = tid; i < n; i += kGT) {
        if (o[i + 1] <= o[i]) continue;   // no observation
        const int f = obs_frame[(size_t)t * obs_capacity + o[i]];
        if (f < 1 || f >= F) continue;    // out of range, or frame 0: not written
        float4 v = points[(size_t)t * map_capacity + i];
        const double X[3] = {(double)v.x, (double)v.y, (double)v.z};
        if (!(std::isfinite(X[0]) && std::isfinite(X[1]) && std::isfinite(X[2]))) continue;
        const double *W = g.prev_R + (n0 + f) * 9, *C = g.prev_T + (n0 + f) * 3, *R = g.R + (n0 + f) * 9, *T = g.T + (n0 + f) * 3;
        const double D[3] = {X[0] - C[0], X[1] - C[1], X[2] - C[2]}, s = g.scale[n0 + f];
        double Y[3], out[3];
#pragma unroll
        for (int k = 0; k < 3; k++) Y[k] = (W[k] * D[0] + W[3 + k] * D[1]) + W[6 + k] * D[2];
#pragma unroll
        for (int r = 0; r < 3; r++) out[r] = s * ((R[3 * r] * Y[0] + R[3 * r + 1] * Y[1]) + R[3 * r + 2] * Y[2]) + T[r];
        v.x = (float)out[0];
        v.y = (float)out[1];
        v.z = (float)out[2];
        points[(size_t)t * map_capacity + i] = v;
    }
}

bool params_ok(const vslam_graph_params &p) {
    return p.max_iterations >= 1 && p.max_iterations <= 64 && p.cg_iterations >= 1 && p.cg_iterations <= 8192 && p.cg_tolerance > 0.0 &&
           p.cg_tolerance < 1.0;
}
}  // namespace

// the launch of vslam_graph_optimize behind its checks; vslam_world_close_loops (below) shares it
static int graph_launch(vslam_ctx *ctx, double *d_scale, double *d_R, double *d_T, const int32_t *d_fixed, const int32_t *d_n_nodes, int batch,
                        int node_stride, const int32_t *d_edge_ab, const double *d_edge_scale, const double *d_edge_R, const double *d_edge_T,
                        const double *d_edge_weight, const int32_t *d_n_edges, int edge_stride, const vslam_graph_params &p, double *d_stats) {
    GraphArgs a;
    a.workspace_item = gr_workspace_bytes(node_stride, edge_stride);
    void *ptr = nullptr;
    int rc;
    if ((rc = vs_arena_get(ctx, "graph_workspace", a.workspace_item * (size_t)batch, &ptr))) return rc;
    a.workspace = static_cast<unsigned char *>(ptr);
    a.scale = d_scale; a.R = d_R; a.T = d_T; a.fixed = d_fixed; a.ab = d_edge_ab; a.n_nodes = d_n_nodes; a.n_edges = d_n_edges;
    a.z_scale = d_edge_scale; a.z_R = d_edge_R; a.z_T = d_edge_T; a.z_w = d_edge_weight;
    a.node_stride = node_stride; a.edge_stride = edge_stride;
    a.stats = d_stats;
    a.prm.max_iterations = p.max_iterations; a.prm.cg_iterations = p.cg_iterations; a.prm.cg_tolerance = p.cg_tolerance;
    VsProfScope ps(ctx, "graph_optimize_kernel");
    graph_optimize_kernel<<<batch, kGT, 0, ctx->stream>>>(a);
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

extern "C" {

int vslam_graph_params_default(vslam_graph_params *out) {
    if (!out) return VSLAM_ERR_INVALID;
    out->max_iterations = 20; out->cg_iterations = 2048; out->cg_tolerance = 1e-8;
    return VSLAM_OK;
}

int vslam_graph_optimize(vslam_ctx *ctx, double *d_scale, double *d_R, double *d_T, const int32_t *d_fixed, const int32_t *d_n_nodes, int batch,
                         int node_stride, const int32_t *d_edge_ab, const double *d_edge_scale, const double *d_edge_R, const double *d_edge_T,
                         const double *d_edge_weight, const int32_t *d_n_edges, int edge_stride, const vslam_graph_params *params,
                         double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, d_scale && d_R && d_T && d_fixed && d_n_nodes && d_edge_ab && d_edge_scale && d_edge_R && d_edge_T && d_edge_weight && d_n_edges,
               VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, batch > 0 && node_stride > 0 && edge_stride > 0, VSLAM_ERR_INVALID);
    vslam_graph_params p;
    vslam_graph_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, params_ok(p), VSLAM_ERR_INVALID);
    VS_ALIGNED(ctx, d_edge_ab, 8);   // int2 rows
    VS_REQUIRE(ctx, vs_ptr_bits(d_scale, d_R, d_T, d_edge_scale, d_edge_R, d_edge_T, d_edge_weight, d_stats) % 8 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_fixed, d_n_nodes, d_n_edges) % 4 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, node_stride <= VSLAM_GRAPH_MAX_NODES && edge_stride <= VSLAM_GRAPH_MAX_EDGES, VSLAM_ERR_CAPACITY);
    return graph_launch(ctx, d_scale, d_R, d_T, d_fixed, d_n_nodes, batch, node_stride, d_edge_ab, d_edge_scale, d_edge_R, d_edge_T, d_edge_weight,
                        d_n_edges, edge_stride, p, d_stats);
}

int vslam_world_close_loops(vslam_ctx *ctx, vslam_world *world, vslam_map *map, const int32_t *d_track, const int32_t *d_frame_a,
                            const int32_t *d_frame_b, const int32_t *d_use, const double *d_scale, const double *d_R, const double *d_T, int loops,
                            const double *seq_weight, const double *loop_weight, const vslam_graph_params *params, double *d_stats) {
    if (!ctx) return VSLAM_ERR_INVALID;
    VS_REQUIRE(ctx, world && map && d_track && d_frame_a && d_frame_b && d_use && d_scale && d_R && d_T, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_world_of_map(ctx, world, map), VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, loops > 0, VSLAM_ERR_INVALID);
    vslam_graph_params p;
    vslam_graph_params_default(&p);
    if (params) p = *params;
    VS_REQUIRE(ctx, params_ok(p), VSLAM_ERR_INVALID);
    WorldGraph g;
    for (int k = 0; k < 3; k++) {
        g.w_seq[k] = seq_weight ? seq_weight[k] : 1.0;
        g.w_loop[k] = loop_weight ? loop_weight[k] : 1.0;
        VS_REQUIRE(ctx, std::isfinite(g.w_seq[k]) && g.w_seq[k] >= 0.0 && std::isfinite(g.w_loop[k]) && g.w_loop[k] >= 0.0, VSLAM_ERR_INVALID);
    }
    VS_REQUIRE(ctx, vs_ptr_bits(d_scale, d_R, d_T, d_stats) % 8 == 0, VSLAM_ERR_INVALID);
    VS_REQUIRE(ctx, vs_ptr_bits(d_track, d_frame_a, d_frame_b, d_use) % 4 == 0, VSLAM_ERR_INVALID);
    vslam_map_arrays m;
    int rc;
    if ((rc = vs_world_map_view(ctx, world, map, &m))) return rc;
    VS_REQUIRE(ctx, m.frames <= VSLAM_GRAPH_MAX_NODES, VSLAM_ERR_CAPACITY);
    const size_t Tr = m.tracks, F = m.frames, P = m.map_capacity, O = m.obs_capacity;
    const size_t Es = std::max<size_t>(1, std::min<size_t>(VSLAM_GRAPH_MAX_EDGES, (F - 1) + (size_t)loops));
    void *ptr = nullptr;
    if ((rc = vs_arena_get(ctx, "graph_world_f64", sizeof(double) * Tr * (F * 25 + Es * 16 + 4), &ptr))) return rc;
    g.scale = static_cast<double *>(ptr);
    g.R = g.scale + Tr * F;
    g.T = g.R + Tr * F * 9;
    g.prev_R = g.T + Tr * F * 3;
    g.prev_T = g.prev_R + Tr * F * 9;
    g.z_scale = g.prev_T + Tr * F * 3;
    g.z_R = g.z_scale + Tr * Es;
    g.z_T = g.z_R + Tr * Es * 9;
    g.z_w = g.z_T + Tr * Es * 3;
    double *stats = g.z_w + Tr * Es * 3;
    if ((rc = vs_arena_get(ctx, "graph_world_i32", sizeof(int32_t) * Tr * (2 * Es + F + 2 + (P + 1) + 2 * O), &ptr))) return rc;
    g.ab = static_cast<int32_t *>(ptr);   // first: int2 rows on 8 bytes
    g.fixed = g.ab + Tr * Es * 2;
    g.n_nodes = g.fixed + Tr * F;
    g.n_edges = g.n_nodes + Tr;
    int32_t *off = g.n_edges + Tr, *obs_frame = off + Tr * (P + 1), *obs_kp = obs_frame + Tr * O;
    g.max_frames = m.max_frames; g.frames = m.frames; g.edge_stride = (int)Es;
    if ((rc = vslam_map_observations(ctx, map, off, obs_frame, obs_kp))) return rc;
    LoopList l{d_track, d_frame_a, d_frame_b, d_use, d_scale, d_R, d_T, loops};
    {
        VsProfScope ps(ctx, "graph_world_gather_kernel");
        graph_world_gather_kernel<<<m.tracks, kGT, 0, ctx->stream>>>(g, l, m.tracks, world->Twc);
    }
    VS_HIP(ctx, hipGetLastError());
    if ((rc = graph_launch(ctx, g.scale, g.R, g.T, g.fixed, g.n_nodes, m.tracks, m.frames, g.ab, g.z_scale, g.z_R, g.z_T, g.z_w, g.n_edges, (int)Es, p,
                           stats)))
        return rc;
    {
        VsProfScope ps(ctx, "graph_world_scatter_kernel");
        graph_world_scatter_kernel<<<m.tracks, kGT, 0, ctx->stream>>>(g, stats, d_stats, world->kp_stride, world->map_capacity, m.obs_capacity,
                                                                      m.d_sizes, off, obs_frame, world->Twc, world->pose, world->scale, world->carry,
                                                                      world->carry_idx, reinterpret_cast<float4 *>(world->world_points));
    }
    VS_HIP(ctx, hipGetLastError());
    return VSLAM_OK;
}

}  // extern "C"
