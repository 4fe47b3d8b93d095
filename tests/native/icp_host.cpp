// Host driver of csrc/kernels/icp_core.h: the launches of icp_kernels.h as serial loops (same chunks, same lane patterns, same
// block partials), reading one problem from a file and writing the point lists and the refinement.  The blocks of a step run
// in forward, reverse or a shuffled order, so the finishing role falls to different blocks.  Built and run by
// tests/test_icp_cpu.py (also with -fsanitize=address,undefined: this is the sanitizer run of the refinement's arithmetic).
//
// problem file (little endian): int32 W, H, crop_rows, crop_cols, mode, max_iterations, n, order; float64 K[9], factor,
//   tolerance; float32 syn[H*W], crop[crop_rows*crop_cols]; int32 sub_syn[n], sub_real[n].   n == 0: points only.
// output file: int32 n_syn, n_real; float64 stats[5] (centroid, radius, thresh); float64 syn_pts[n_syn*3], real_pts[n_real*3];
//   then for n > 0: int32 error, i; float64 mean_error, T[16], d2[n]; int32 idx[n]; float64 src[n*3].
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../augmentedautoencoder_amd/csrc/kernels/icp_core.h"

using namespace aae_icp;

template <typename T>
static void rd(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "icp_host: short problem file\n");
        exit(2);
    }
}

static const int kChunk = 256;

// icp_points<false> + icp_points<true>
static int points(const std::vector<float>& depth, int w, int h, const IcpCamera& cam, const double* stats, std::vector<double>* out) {
    const int npix = w * h, nchunks = (npix + kChunk - 1) / kChunk;
    std::vector<int> counts(nchunks, 0);
    auto keeps = [&](int i, double* pt) {
        if (!icp_is_point(depth[i])) return false;
        icp_backproject(cam, i % w, i / w, depth[i], pt);
        return stats ? icp_filter_keeps(pt, stats, stats[4]) : true;
    };
    double pt[3];
    for (int c = 0; c < nchunks; ++c)
        for (int i = c * kChunk; i < npix && i < (c + 1) * kChunk; ++i) counts[c] += keeps(i, pt) ? 1 : 0;
    out->assign((size_t)npix * 3, -12345.0);
    int total = 0;
    for (int c = nchunks - 1; c >= 0; --c) {                     // chunks in any order: each finds its own place
        int rank = 0;
        for (int k = 0; k < c; ++k) rank += counts[k];
        for (int i = c * kChunk; i < npix && i < (c + 1) * kChunk; ++i)
            if (keeps(i, pt)) {
                if (rank >= npix) exit(3);
                for (int k = 0; k < 3; ++k) (*out)[(size_t)rank * 3 + k] = pt[k];
                ++rank;
            }
        if (c == nchunks - 1) total = rank;
    }
    out->resize((size_t)total * 3);
    return total;
}

// icp_stats
static void stats_of(const std::vector<double>& P, int n, double factor, double* st) {
    double acc[3][ICP_LANES];
    for (int t = 0; t < ICP_LANES; ++t) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = t; i < n; i += ICP_LANES) { s0 += P[3 * (size_t)i]; s1 += P[3 * (size_t)i + 1]; s2 += P[3 * (size_t)i + 2]; }
        acc[0][t] = s0; acc[1][t] = s1; acc[2][t] = s2;
    }
    for (int k = 0; k < 3; ++k) {
        icp_tree_sum(acc[k]);
        st[k] = acc[k][0] / (double)n;
    }
    double m = 0.0;
    for (int i = 0; i < n; ++i) {
        const double d2 = icp_dist2(P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2], st[0], st[1], st[2]);
        m = d2 > m ? d2 : m;
    }
    st[3] = sqrt(m);
    st[4] = factor * st[3];
}

static int clamp_index(int idx, int count, int* err) {
    int hi = count;
    if (hi < 1) { *err |= ICP_ERR_INDEX; hi = 1; }
    if (idx < 0 || idx >= hi) { *err |= ICP_ERR_INDEX; idx = idx < 0 ? 0 : hi - 1; }
    return idx;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: icp_host <problem.bin> <out.bin>\n");
        return 1;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t hd[8];
    rd(in, hd, 8);
    const int W = hd[0], H = hd[1], ch = hd[2], cw = hd[3], mode = hd[4], max_it = hd[5], n = hd[6], order = hd[7];
    if (W < 1 || H < 1 || ch < 1 || cw < 1 || W > 4096 || H > 4096 || ch > 4096 || cw > 4096 || n < 0 || n > ICP_MAX_POINTS || (n > 0 && n < 3) || max_it < 1 ||
        max_it > 1000)
        return 1;
    double K[9], ft[2];
    rd(in, K, 9); rd(in, ft, 2);
    std::vector<float> syn((size_t)W * H), crop((size_t)ch * cw);
    rd(in, syn.data(), syn.size()); rd(in, crop.data(), crop.size());
    std::vector<int32_t> sub_syn(n), sub_real(n);
    rd(in, sub_syn.data(), sub_syn.size()); rd(in, sub_real.data(), sub_real.size());
    fclose(in);

    IcpCamera cam = {K[0], K[2], K[4], K[5]};
    std::vector<double> syn_pts, real_pts;
    const int32_t n_syn = points(syn, W, H, cam, nullptr, &syn_pts);
    double st[5];
    stats_of(syn_pts, n_syn, ft[0], st);
    IcpCamera ccam = cam;
    ccam.K02 = (double)(ch / 2);
    ccam.K12 = (double)(cw / 2);
    const int32_t n_real = points(crop, cw, ch, ccam, st, &real_pts);
    fwrite(&n_syn, 4, 1, out); fwrite(&n_real, 4, 1, out);
    fwrite(st, 8, 5, out);
    fwrite(syn_pts.data(), 8, syn_pts.size(), out);
    fwrite(real_pts.data(), 8, real_pts.size(), out);
    if (n == 0) {
        fclose(out);
        return 0;
    }

    // icp_gather (slot 0 of an empty list reads as 0 here; the device reads whatever the workspace holds there)
    if (syn_pts.empty()) syn_pts.assign(3, 0.0);
    if (real_pts.empty()) real_pts.assign(3, 0.0);
    int32_t err = 0;
    std::vector<double> src((size_t)n * 3), orig((size_t)n * 3), dst((size_t)n * 3);
    for (int i = 0; i < n; ++i) {
        const int is = clamp_index(sub_syn[i], n_syn, &err), ir = clamp_index(sub_real[i], n_real, &err);
        for (int k = 0; k < 3; ++k) {
            src[(size_t)i * 3 + k] = orig[(size_t)i * 3 + k] = syn_pts[(size_t)is * 3 + k];
            dst[(size_t)i * 3 + k] = real_pts[(size_t)ir * 3 + k];
        }
    }

    // icp_step x max_iterations
    const int nblk = (n + ICP_BLOCK_POINTS - 1) / ICP_BLOCK_POINTS;
    std::vector<int> blocks(nblk);
    for (int b = 0; b < nblk; ++b) blocks[b] = order == 1 ? nblk - 1 - b : b;
    if (order == 2) {
        uint32_t lcg = 12345u;
        for (int b = nblk - 1; b > 0; --b) {
            lcg = lcg * 1664525u + 1013904223u;
            const int j = (int)((lcg >> 8) % (uint32_t)(b + 1));
            const int t = blocks[b]; blocks[b] = blocks[j]; blocks[j] = t;
        }
    }
    IcpState state = {0.0, 0.0, 0, 0};
    std::vector<double> partials((size_t)nblk * ICP_NQ, -7.0), d2s(n, -1.0);
    std::vector<int32_t> idxs(n, -1);
    for (int it = 0; it < max_it; ++it) {
        if (state.done) continue;                                 // the launches behind convergence do nothing
        for (int turn = 0; turn < nblk; ++turn) {
            const int bx = blocks[turn];
            const int cnt = n - bx * ICP_BLOCK_POINTS < ICP_BLOCK_POINTS ? n - bx * ICP_BLOCK_POINTS : ICP_BLOCK_POINTS;
            double q[ICP_BLOCK_POINTS][ICP_NQ];
            for (int k = 0; k < cnt; ++k) {
                const int i = bx * ICP_BLOCK_POINTS + k;
                const double* s = &src[(size_t)i * 3];
                double best = HUGE_VAL;
                int bi = 0;
                for (int j = n - 1; j >= 0; --j) {                // any scan order: the key decides
                    const double d2 = icp_dist2(s[0], s[1], s[2], dst[(size_t)j * 3], dst[(size_t)j * 3 + 1], dst[(size_t)j * 3 + 2]);
                    if (icp_key_less(d2, j, best, bi)) { best = d2; bi = j; }
                }
                icp_pair_terms(s, &dst[(size_t)bi * 3], st, sqrt(best), q[k]);
                d2s[i] = best;
                idxs[i] = bi;
            }
            for (int u = 0; u < ICP_NQ; ++u) {
                double sum = 0.0;
                for (int k = 0; k < cnt; ++k) sum += q[k][u];
                partials[(size_t)bx * ICP_NQ + u] = sum;
            }
            if (turn != nblk - 1) continue;
            // the last block to arrive finishes: partials in block order, solve, move the source points, advance
            double S[ICP_NQ], T[16];
            for (int u = 0; u < ICP_NQ; ++u) {
                double sum = 0.0;
                for (int b = 0; b < nblk; ++b) sum += partials[(size_t)b * ICP_NQ + u];
                S[u] = sum;
            }
            const double mean = icp_solve(S, n, st, mode, T);
            icp_advance(&state, mean, ft[1], max_it);
            for (int i = 0; i < n; ++i) icp_apply(T, &src[(size_t)i * 3]);
        }
    }

    // icp_finish
    double acc[ICP_NQ][ICP_LANES];
    for (int t = 0; t < ICP_LANES; ++t) {
        double s[ICP_NQ];
        for (int u = 0; u < ICP_NQ; ++u) s[u] = 0.0;
        for (int i = t; i < n; i += ICP_LANES) {
            double q[ICP_NQ];
            icp_pair_terms(&orig[(size_t)i * 3], &src[(size_t)i * 3], st, 0.0, q);
            for (int u = 0; u < ICP_NQ; ++u) s[u] += q[u];
        }
        for (int u = 0; u < ICP_NQ; ++u) acc[u][t] = s[u];
    }
    double S[ICP_NQ], T[16];
    for (int u = 0; u < ICP_NQ; ++u) {
        icp_tree_sum(acc[u]);
        S[u] = acc[u][0];
    }
    icp_solve(S, n, st, mode, T);
    const int32_t i_ref = state.iterations - 1;
    fwrite(&err, 4, 1, out); fwrite(&i_ref, 4, 1, out);
    fwrite(&state.mean_error, 8, 1, out);
    fwrite(T, 8, 16, out);
    fwrite(d2s.data(), 8, d2s.size(), out);
    fwrite(idxs.data(), 4, idxs.size(), out);
    fwrite(src.data(), 8, src.size(), out);
    fclose(out);
    return 0;
}
