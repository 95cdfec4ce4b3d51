// Optimal matching of picks to target centres (reference evaluation/algorithms.py:6-21, match_coordinates), DESIGN.md 4.21.
//
// cost[i][j] = min(|pred_i - target_j|^2 - radius^3, 0) in float64 (the CUBE of the radius is the reference's), and the
// result is a rectangular assignment of minimum total cost: shortest augmenting paths with dual variables, the method
// scipy.optimize.linear_sum_assignment runs.  The cost matrix is never written: a cost is recomputed from the two
// coordinate rows wherever it is needed.
//
// One workgroup per image.  The SHORTER side of the rectangle gives the rows (nr <= nc), as scipy transposes.  Thread t owns
// the columns t, t + B, t + 2 B, t + 3 B (B = block size): their dual v, their shortest-path cost and their "scanned" bit
// live in its registers; path[], row4col[] and the columns' coordinates are in LDS; a row's {x, y, z, u} and col4row[] are
// in LDS where they fit beside the columns and in the workspace otherwise (one generic pointer, one code path).
#include "common.h"

namespace {

constexpr int MATCH_MAX = 4096;            // picks and targets per image
constexpr int MATCH_CPT = 4;               // columns per thread
constexpr int MATCH_LDS_MAX = 160 * 1024 - 1024;     // one workgroup may take the CU's LDS; 1 KiB left to the static arrays
constexpr unsigned MATCH_ASSIGNED = 1u << 13;        // tie key: free columns first, then the lower column

struct MatchLayout {            // dynamic LDS, in bytes from its base; NC, NR even
    int NC, NR, rows_in_lds;
    size_t col_xyz, row_state, path, row4col, col4row, total;
};

inline MatchLayout match_layout(int max_nc, int max_nr) {
    MatchLayout L;
    L.NC = (max_nc + 1) & ~1;
    L.NR = (max_nr + 1) & ~1;
    const size_t cols = (size_t)L.NC * (3 * sizeof(double) + 2 * sizeof(int));
    const size_t rows = (size_t)L.NR * (4 * sizeof(double) + sizeof(int));
    L.rows_in_lds = cols + rows <= (size_t)MATCH_LDS_MAX;
    L.col_xyz = 0;
    L.row_state = (size_t)L.NC * 3 * sizeof(double);
    L.path = L.row_state + (L.rows_in_lds ? (size_t)L.NR * 4 * sizeof(double) : 0);
    L.row4col = L.path + (size_t)L.NC * sizeof(int);
    L.col4row = L.row4col + (size_t)L.NC * sizeof(int);
    L.total = L.col4row + (L.rows_in_lds ? (size_t)L.NR * sizeof(int) : 0);
    return L;
}

// workspace: [0, hdr) the two offset tables (int, n_img + 1 each); then per image a row-state block {x, y, z, u}[NR]
// followed by col4row[NR], used where the rows do not fit in LDS
inline size_t match_hdr_bytes(int n_img) { return mi_align_up(2 * ((size_t)n_img + 1) * sizeof(int), 256); }
inline size_t match_image_bytes(int nr) { return mi_align_up((size_t)((nr + 1) & ~1) * (4 * sizeof(double) + sizeof(int)), 256); }

// d2 as numpy evaluates it: every product and sum rounded on its own, (dx^2 + dy^2) + dz^2.  A fused multiply-add would
// round differently for coordinates that are not integers, and dist is promised to be sqrt of the reference's d2.
__device__ __forceinline__ double match_d2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

__device__ __forceinline__ double match_cost(double ax, double ay, double az, double bx, double by, double bz, double r3) {
    const double c = match_d2(ax, ay, az, bx, by, bz) - r3;
    return c < 0.0 ? c : 0.0;              // a NaN becomes 0: no cost is ever NaN
}

__global__ __launch_bounds__(1024) void match_kernel(const double* __restrict__ preds, const double* __restrict__ targets,
                                                     const int* __restrict__ pred_off, const int* __restrict__ targ_off,
                                                     double radius, int* __restrict__ pred_to_target, double* __restrict__ dist,
                                                     double* __restrict__ total_cost, unsigned char* __restrict__ ws_rows,
                                                     size_t ws_image_bytes, MatchLayout L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char match_lds[];
    __shared__ double red_val[2][16];
    __shared__ unsigned red_key[2][16];

    const int img = blockIdx.x, tid = threadIdx.x, B = blockDim.x, lane = tid & 63, wave = tid >> 6, n_waves = B >> 6;
    const int p0 = pred_off[img], P = pred_off[img + 1] - p0;
    const int t0 = targ_off[img], T = targ_off[img + 1] - t0;
    const double r3 = radius * radius * radius;
    const bool rows_are_preds = P <= T;
    const int nr = rows_are_preds ? P : T, nc = rows_are_preds ? T : P;
    const double* rsrc = rows_are_preds ? preds + 3 * (size_t)p0 : targets + 3 * (size_t)t0;
    const double* csrc = rows_are_preds ? targets + 3 * (size_t)t0 : preds + 3 * (size_t)p0;

    for (int i = tid; i < P; i += B) {     // <= P / B trips
        pred_to_target[p0 + i] = -1;
        dist[p0 + i] = 0.0;
    }
    // the entry refuses these sizes; a kernel that met them would index past its arrays
    if (nr == 0 || nc > L.NC || nr > L.NR || nc > MATCH_CPT * B) {
        if (tid == 0) total_cost[img] = 0.0;
        return;
    }

    double* cx = (double*)(match_lds + L.col_xyz);
    double* cy = cx + L.NC;
    double* cz = cy + L.NC;
    int* path = (int*)(match_lds + L.path);
    int* row4col = (int*)(match_lds + L.row4col);
    double* rowst;                          // {x, y, z, u} per row: LDS or workspace behind one generic pointer
    int* col4row;
    if (L.rows_in_lds) {
        rowst = (double*)(match_lds + L.row_state);
        col4row = (int*)(match_lds + L.col4row);
    } else {
        rowst = (double*)(ws_rows + (size_t)img * ws_image_bytes);
        col4row = (int*)(rowst + 4 * (size_t)L.NR);
    }

    for (int j = tid; j < nc; j += B) {    // <= MATCH_CPT trips
        cx[j] = csrc[3 * j];
        cy[j] = csrc[3 * j + 1];
        cz[j] = csrc[3 * j + 2];
        row4col[j] = -1;
        path[j] = -1;
    }
    for (int i = tid; i < nr; i += B) {    // <= nr / B trips
        rowst[4 * i] = rsrc[3 * i];
        rowst[4 * i + 1] = rsrc[3 * i + 1];
        rowst[4 * i + 2] = rsrc[3 * i + 2];
        rowst[4 * i + 3] = 0.0;
        col4row[i] = -1;
    }
    double v[MATCH_CPT], sp[MATCH_CPT];
    bool scanned[MATCH_CPT];
#pragma unroll
    for (int k = 0; k < MATCH_CPT; ++k) v[k] = 0.0;
    __syncthreads();

    int parity = 0;
    for (int cur = 0; cur < nr; ++cur) {   // nr trips: one augmentation per row
#pragma unroll
        for (int k = 0; k < MATCH_CPT; ++k) {
            sp[k] = INFINITY;
            scanned[k] = false;
        }
        double min_val = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step < nc && sink < 0; ++step) {      // <= nc trips: every trip moves one column into the scanned set
            const double rx = rowst[4 * i], ry = rowst[4 * i + 1], rz = rowst[4 * i + 2], ui = rowst[4 * i + 3];
            double best = INFINITY;
            unsigned key = 0xffffffffu;
#pragma unroll
            for (int k = 0; k < MATCH_CPT; ++k) {
                const int j = tid + k * B;
                if (j < nc && !scanned[k]) {
                    const double r = min_val + match_cost(rx, ry, rz, cx[j], cy[j], cz[j], r3) - ui - v[k];
                    if (r < sp[k]) {
                        sp[k] = r;
                        path[j] = i;
                    }
                    const unsigned kj = (row4col[j] >= 0 ? MATCH_ASSIGNED : 0u) | (unsigned)j;
                    if (sp[k] < best || (sp[k] == best && kj < key)) {
                        best = sp[k];
                        key = kj;
                    }
                }
            }
            // arg-min of (value, key): inside the wave, then across the waves
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const unsigned ok = __shfl_xor(key, o, 64);
                if (ob < best || (ob == best && ok < key)) {
                    best = ob;
                    key = ok;
                }
            }
            if (lane == 0) {
                red_val[parity][wave] = best;
                red_key[parity][wave] = key;
            }
            __syncthreads();               // also orders this trip's path[] writes in front of the walk below
            best = red_val[parity][0];
            key = red_key[parity][0];
            for (int w = 1; w < n_waves; ++w) {          // <= 16 trips
                const double ob = red_val[parity][w];
                const unsigned ok = red_key[parity][w];
                if (ob < best || (ob == best && ok < key)) {
                    best = ob;
                    key = ok;
                }
            }
            parity ^= 1;                   // the next trip writes the other pair of arrays: no second barrier
            if (key == 0xffffffffu) break; // no column left (cannot happen while nr <= nc); uniform
            const int bj = (int)(key & (MATCH_ASSIGNED - 1));
            min_val = best;
#pragma unroll
            for (int k = 0; k < MATCH_CPT; ++k)
                if (tid + k * B == bj) scanned[k] = true;
            const int owner = row4col[bj];
            if (owner < 0) sink = bj;
            else i = owner;
        }
        if (sink < 0) break;               // uniform; only on the impossible exit above

        // duals, once per augmentation (every scanned column but the sink has a row in the tree)
#pragma unroll
        for (int k = 0; k < MATCH_CPT; ++k) {
            const int j = tid + k * B;
            if (j < nc && scanned[k]) {
                const double d = min_val - sp[k];
                v[k] -= d;
                const int ri = row4col[j];
                if (ri >= 0) rowst[4 * ri + 3] += d;
            }
        }
        if (tid == 0) rowst[4 * cur + 3] += min_val;
        __syncthreads();
        if (tid == 0) {
            int j = sink;
            for (int step = 0; step < nr; ++step) {      // <= nr trips: the path visits a row once
                if (j < 0 || j >= nc) break;
                const int ri = path[j];
                if (ri < 0 || ri >= nr) break;
                row4col[j] = ri;
                const int nj = col4row[ri];
                col4row[ri] = j;
                j = nj;
                if (ri == cur) break;
            }
        }
        __syncthreads();
    }

    // outputs and the total, rows in order
    double sum = 0.0;
    for (int i = tid; i < nr; i += B) {    // <= nr / B trips
        const int j = col4row[i];
        if (j < 0 || j >= nc) continue;
        const double d2 = match_d2(rowst[4 * i], rowst[4 * i + 1], rowst[4 * i + 2], cx[j], cy[j], cz[j]);
        const double c = d2 - r3;
        if (c < 0.0) {
            sum += c;
            const int p = rows_are_preds ? i : j, t = rows_are_preds ? j : i;
            pred_to_target[p0 + p] = t;
            dist[p0 + p] = sqrt(d2);
        }
    }
    sum = wave_sum(sum);
    __syncthreads();                       // the arg-min arrays are free again
    if (lane == 0) red_val[0][wave] = sum;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < n_waves; ++w) s += red_val[0][w];   // <= 16 trips
        total_cost[img] = s;
    }
}

}  // namespace

extern "C" size_t mi_match_workspace_bytes(int n_img, int max_P, int max_T) {
    if (n_img < 0 || max_P < 0 || max_T < 0 || max_P > MATCH_MAX || max_T > MATCH_MAX) return 0;
    return match_hdr_bytes(n_img) + (size_t)n_img * match_image_bytes(max_P < max_T ? max_P : max_T);
}

extern "C" int mi_match_coordinates(const double* preds, const double* targets, const int* pred_off, const int* targ_off, int n_img,
                                    double radius, int* pred_to_target, double* dist, double* total_cost, void* workspace,
                                    size_t workspace_bytes, mi_stream_t stream) {
    if (n_img < 0 || !pred_off || !targ_off) return MI_E_ARG;
    if (n_img == 0) return MI_OK;
    if (!total_cost || !workspace || !(radius == radius)) return MI_E_ARG;
    if (pred_off[0] < 0 || targ_off[0] < 0) return MI_E_ARG;
    int max_nc = 0, max_nr = 0;
    for (int i = 0; i < n_img; ++i) {
        const long P = (long)pred_off[i + 1] - pred_off[i], T = (long)targ_off[i + 1] - targ_off[i];
        if (P < 0 || T < 0) return MI_E_ARG;
        if (P > MATCH_MAX || T > MATCH_MAX) return MI_E_UNSUPPORTED;      // never truncated: refused before any launch
        const int nr = (int)(P < T ? P : T), nc = (int)(P < T ? T : P);
        if (nr > max_nr) max_nr = nr;
        if (nc > max_nc) max_nc = nc;
    }
    if (pred_off[n_img] > 0 && (!preds || !pred_to_target || !dist)) return MI_E_ARG;
    if (targ_off[n_img] > 0 && !targets) return MI_E_ARG;
    const size_t hdr = match_hdr_bytes(n_img), per_image = match_image_bytes(max_nr);
    if (workspace_bytes < hdr + (size_t)n_img * per_image) return MI_E_WORKSPACE;

    const MatchLayout L = match_layout(max_nc, max_nr);
    if (L.total > (size_t)MATCH_LDS_MAX) return MI_E_UNSUPPORTED;
    static std::atomic<bool> lds_done[64];
    const int rc = mi_allow_dynamic_lds(lds_done, MATCH_LDS_MAX, match_kernel);
    if (rc != MI_OK) return rc;

    const hipStream_t s = (hipStream_t)stream;
    int* d_off = (int*)workspace;
    // the sources are pageable host arrays: the copies have taken them when the calls return
    MI_HIP(hipMemcpyAsync(d_off, pred_off, ((size_t)n_img + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    MI_HIP(hipMemcpyAsync(d_off + n_img + 1, targ_off, ((size_t)n_img + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    const int threads = max_nc <= MATCH_CPT * 256 ? 256 : 1024;
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)n_img), dim3(threads), L.total, s, preds, targets, d_off, d_off + n_img + 1, radius,
                       pred_to_target, dist, total_cost, (unsigned char*)workspace + hdr, per_image, L);
    MI_RETURN_IF_LAUNCH_FAILED();
    return MI_OK;
}
