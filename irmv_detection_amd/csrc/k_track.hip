// Armor tracks (include/irmv_hip.h, "armor tracks"): the track table's step over the frames of one launch.  A module of its
// own, compiled with -ffp-contract=off: every fp64 operation is the one written (track_math.hpp), in the written order, and
// irmv_detection_amd/tracks.py follows it operation for operation.  No reduction whose order depends on the launch shape: the
// only reduction is an arg-min over (d2, track, record) keys, which is exact under any order.
//
// ONE workgroup of 256 threads walks the launch's frames in index order; the table lives in LDS for the launch.  Per frame:
//   load      the frame's stamp against the table's: a stamp that does not rise refuses the frame (uniform branch)
//   measure   thread i < n: record i's eligibility, z and rotated noise -> LDS;  thread k < 32: track k predicted in LDS
//   gate      the 32 n (track, record) pairs dealt over the threads, entry e = record * 32 + track: d2 or +inf -> LDS
//   assign    per round every thread takes the least key of its entries, the waves reduce by __shfl_xor, the four wave
//             winners meet in LDS; the winner's row and column become +inf.  At most min(32, n) rounds, two barriers each.
//   update    thread k < 32: the Kalman update of an assigned track, or its miss and deletion
//   births    thread 0 deals the free entries and ids to the unassigned eligible records in index order (the one serial part:
//             at most 256 flag reads and 32 grants); thread i then fills its own entry
//   store     the records, the header, the snapshot and the table
// What bounds it: latency on one CU.  A frame is ~ 8 barriers plus two per assignment; the fp64 work is 32 n pair distances
// (~ 60 operations and 6 divisions each) over 256 lanes and one 6 x 6 predict / update per track on 32 lanes.
#include <hip/hip_runtime.h>

#include "irmv_common.hpp"
#include "track_math.hpp"

namespace irmv {

static_assert(kTrackCap == 32 && kTrackThreads == 256 && kMaxDetCap <= kTrackThreads, "one thread per record, entry = record * 32 + track");
static_assert(sizeof(DevTrack) % 8 == 0 && sizeof(DevTrackFrame) % 8 == 0 && sizeof(DevTrackTable) == 16 + kTrackCap * sizeof(DevTrack), "copied as 8-byte words");

struct TrackShared {
    DevTrack tab[kTrackCap];
    double d2[kTrackCap * kMaxDetCap];
    double z[kMaxDetCap][3], R6[kMaxDetCap][6], obs_d2[kMaxDetCap];
    int32_t elig[kMaxDetCap], ocls[kMaxDetCap], obs_trk[kMaxDetCap], grant[kMaxDetCap];
    uint32_t grant_id[kMaxDetCap];
    int32_t trk_det[kTrackCap], deleted[kTrackCap];
    double red_d[kTrackThreads / 64];
    int32_t red_i[kTrackThreads / 64];
    double stamp;
    int32_t stamped, n_started, n_no_room;
    uint32_t next_id;
};

__device__ inline bool key_less(double ad, int ai, double bd, int bi) { return ad < bd || (ad == bd && ai < bi); }

__global__ __launch_bounds__(kTrackThreads) void track_kernel(TrackArgs a, int batch)
{
    __shared__ TrackShared sh;
    const int tid = threadIdx.x;
    const double inf = __builtin_huge_val();
    const TrackOpts opt = *a.opts;
    {
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(a.table->tracks);
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(sh.tab);
        for (int w = tid; w < (int)(sizeof(sh.tab) / 8); w += kTrackThreads) dst[w] = src[w];
        if (tid == 0) { sh.stamp = a.table->stamp; sh.stamped = a.table->stamped; sh.next_id = a.table->next_id; }
    }
    __syncthreads();
    bool advanced = false;
    for (int b = 0; b < batch; b++) {
        const TrackSlot *slot = a.slots + a.first + b;
        const double t = slot->stamp;
        int n;
        if (a.dets) n = min(max(a.num_dets[(size_t)b * a.num_dets_stride], 0), a.max_det);
        else n = min(max(a.n_obs, 0), kMaxDetCap);
        n = min(n, kMaxDetCap);
        DevDetTrack *out_det = a.out_det ? a.out_det + (size_t)b * a.max_det : nullptr;
        DevTrackSnap *snap = a.out_snap ? a.out_snap + b : nullptr;
        const bool refuse = (sh.stamped && !(t > sh.stamp)) || !trk_finite(t);   // uniform: LDS values every thread reads alike
        DevDetTrack rec{};   // thread i < n: record i
        if (!refuse) {
            advanced = true;
            // ---- measure and predict
            if (tid < n) {
                int cls, valid;
                double tv[3], C[9];
                bool has_cov = false;
                if (a.dets) {
                    const DevDet &d = a.dets[(size_t)b * a.max_det + tid];
                    cls = (d.cls >= 0 && d.cls < kTrackClasses) ? d.cls : kTrackClasses;   // irmv_det.class_id
                    valid = d.pnp_ok == 1 && d.armor_valid == 1;
                    tv[0] = d.tvec[0]; tv[1] = d.tvec[1]; tv[2] = d.tvec[2];
                    if (a.cov) {
                        const DevPoseCov &pc = a.cov[(size_t)b * a.max_det + tid];
                        if (pc.state == 1) {
                            has_cov = true;
                            C[0] = pc.cov[15]; C[1] = pc.cov[16]; C[2] = pc.cov[17];
                            C[3] = pc.cov[16]; C[4] = pc.cov[18]; C[5] = pc.cov[19];
                            C[6] = pc.cov[17]; C[7] = pc.cov[19]; C[8] = pc.cov[20];
                        }
                    }
                } else {
                    const TrackObs &o = a.obs[tid];
                    cls = o.cls; valid = o.valid == 1;
                    tv[0] = o.tvec[0]; tv[1] = o.tvec[1]; tv[2] = o.tvec[2];
                    if (o.has_cov == 1) {
                        has_cov = true;
#pragma unroll
                        for (int i = 0; i < 9; i++) C[i] = o.cov[i];
                    }
                }
                if (!has_cov) trk_default_noise(tv[2], opt.sigma_lat, opt.sigma_rng, C);
                double z[3], R6[6];
                const bool ok = valid && trk_measure(tv, C, slot->R, slot->t, z, R6);
                sh.elig[tid] = ok; sh.ocls[tid] = cls; sh.obs_trk[tid] = -1; sh.grant[tid] = -1; sh.obs_d2[tid] = 0.0;
                for (int i = 0; i < 3; i++) sh.z[tid][i] = ok ? z[i] : 0.0;
                for (int i = 0; i < 6; i++) sh.R6[tid][i] = ok ? R6[i] : 0.0;
            }
            if (tid < kTrackCap) {
                sh.trk_det[tid] = -1; sh.deleted[tid] = 0;
                DevTrack &tr = sh.tab[tid];
                if (sh.stamped && tr.state != 0) {
                    trk_predict(tr.x, tr.P, t - sh.stamp, opt.accel_sigma);
                    tr.stamp = t;
                }
            }
            __syncthreads();
            // ---- gate
            const int entries = n * kTrackCap;
            for (int e = tid; e < entries; e += kTrackThreads) {
                const int k = e & (kTrackCap - 1), i = e / kTrackCap;
                const DevTrack &tr = sh.tab[k];
                double d = inf;
                if (tr.state != 0 && sh.elig[i] && (opt.match_class == 0 || sh.ocls[i] == tr.cls)) {
                    double y[3], Si6[6];
                    if (trk_innovation(tr.x, tr.P, sh.z[i], sh.R6[i], y, Si6)) {
                        const double v = trk_distance2(y, Si6);
                        if (v >= 0.0 && v <= opt.gate) d = v;
                    }
                }
                sh.d2[e] = d;
            }
            __syncthreads();
            // ---- assign: the least (d2, track, record) of what is left, until nothing is
            for (int round = 0; round < kTrackCap; round++) {
                double bd = inf;
                int bi = 0x7fffffff;
                for (int e = tid; e < entries; e += kTrackThreads) {
                    const double d = sh.d2[e];
                    const int key = (e & (kTrackCap - 1)) * kMaxDetCap + e / kTrackCap;
                    if (key_less(d, key, bd, bi)) { bd = d; bi = key; }
                }
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) {
                    const double od = __shfl_xor(bd, m);
                    const int oi = __shfl_xor(bi, m);
                    if (key_less(od, oi, bd, bi)) { bd = od; bi = oi; }
                }
                if ((tid & 63) == 0) { sh.red_d[tid >> 6] = bd; sh.red_i[tid >> 6] = bi; }
                __syncthreads();
                bd = sh.red_d[0]; bi = sh.red_i[0];
#pragma unroll
                for (int w = 1; w < kTrackThreads / 64; w++)
                    if (key_less(sh.red_d[w], sh.red_i[w], bd, bi)) { bd = sh.red_d[w]; bi = sh.red_i[w]; }
                if (!(bd < inf)) break;   // uniform: every thread has read the same four
                const int k = bi / kMaxDetCap, i = bi % kMaxDetCap;
                if (tid == 0) { sh.trk_det[k] = i; sh.obs_trk[i] = k; sh.obs_d2[i] = bd; }
                if (tid < n) sh.d2[tid * kTrackCap + k] = inf;
                if (tid < kTrackCap) sh.d2[i * kTrackCap + tid] = inf;
                __syncthreads();
            }
            __syncthreads();
            // ---- update, misses and deletion
            if (tid < kTrackCap) {
                DevTrack &tr = sh.tab[tid];
                if (tr.state != 0) {
                    const int i = sh.trk_det[tid];
                    if (i >= 0) {
                        double y[3], Si6[6];
                        (void)trk_innovation(tr.x, tr.P, sh.z[i], sh.R6[i], y, Si6);
                        trk_update(tr.x, tr.P, y, Si6);
                        tr.hits = tr.hits + 1;
                        tr.misses = 0;
                        tr.last_hit = t;
                        if (tr.hits >= opt.confirm_hits) tr.state = 2;
                    } else {
                        tr.misses = tr.misses + 1;
                        if (tr.misses > opt.max_misses || (t - tr.last_hit) > opt.max_coast_s) {
                            unsigned long long *w = reinterpret_cast<unsigned long long *>(&tr);
                            for (int q = 0; q < (int)(sizeof(DevTrack) / 8); q++) w[q] = 0ull;
                            sh.deleted[tid] = 1;
                        }
                    }
                }
            }
            __syncthreads();
            // ---- births: thread 0 deals entries and ids in record order
            if (tid == 0) {
                int k = 0, started = 0, no_room = 0;
                uint32_t id = sh.next_id;
                for (int i = 0; i < n; i++) {
                    if (!sh.elig[i] || sh.obs_trk[i] >= 0) continue;
                    while (k < kTrackCap && sh.tab[k].state != 0) k++;
                    if (k == kTrackCap) { sh.grant[i] = -2; no_room++; continue; }
                    sh.grant[i] = k; sh.grant_id[i] = id++;
                    sh.trk_det[k] = i;
                    k++; started++;
                }
                sh.next_id = id; sh.n_started = started; sh.n_no_room = no_room;
            }
            __syncthreads();
            if (tid < n) {
                const int k = sh.obs_trk[tid], g = sh.grant[tid];
                if (k >= 0) {
                    const DevTrack &tr = sh.tab[k];
                    rec.state = 1; rec.track = k; rec.id = tr.id; rec.hits = tr.hits; rec.d2 = sh.obs_d2[tid];
                    for (int i = 0; i < 3; i++) { rec.pos[i] = tr.x[i]; rec.vel[i] = tr.x[3 + i]; }
                } else if (g >= 0) {
                    DevTrack &tr = sh.tab[g];
                    tr.id = sh.grant_id[tid]; tr.cls = sh.ocls[tid]; tr.state = opt.confirm_hits <= 1 ? 2 : 1;
                    tr.hits = 1; tr.misses = 0; tr.det = 0;
                    tr.first = t; tr.last_hit = t; tr.stamp = t;
                    const double v2 = opt.init_vel_sigma * opt.init_vel_sigma;
                    for (int i = 0; i < 36; i++) tr.P[i] = 0.0;
                    for (int i = 0; i < 3; i++) { tr.x[i] = sh.z[tid][i]; tr.x[3 + i] = 0.0; tr.P[(3 + i) * 7] = v2; }
                    const double *r = sh.R6[tid];
                    tr.P[0] = r[0]; tr.P[1] = r[1]; tr.P[2] = r[2];
                    tr.P[6] = r[1]; tr.P[7] = r[3]; tr.P[8] = r[4];
                    tr.P[12] = r[2]; tr.P[13] = r[4]; tr.P[14] = r[5];
                    rec.state = 2; rec.track = g; rec.id = tr.id; rec.hits = 1;
                    for (int i = 0; i < 3; i++) rec.pos[i] = sh.z[tid][i];
                } else if (g == -2) {
                    rec.state = -1; rec.track = -1;
                }
            }
            __syncthreads();
            if (tid == 0) { sh.stamp = t; sh.stamped = 1; }
        }
        // ---- store (a refused frame: zero records, the table as it is)
        if (tid < kTrackCap) sh.tab[tid].det = refuse ? -1 : sh.trk_det[tid];
        if (tid < n && out_det) out_det[tid] = rec;
        __syncthreads();
        if (snap) {
            if (tid == 0) {
                DevTrackFrame f{};
                f.stamp = t; f.next_id = sh.next_id;
                if (refuse) f.state = -2;
                else {
                    f.state = 1; f.n_started = sh.n_started; f.n_no_room = sh.n_no_room;
                    for (int k = 0; k < kTrackCap; k++) {
                        f.n_live += sh.tab[k].state != 0; f.n_confirmed += sh.tab[k].state == 2; f.n_deleted += sh.deleted[k];
                    }
                }
                snap->frame = f;
            }
            const unsigned long long *src = reinterpret_cast<const unsigned long long *>(sh.tab);
            unsigned long long *dst = reinterpret_cast<unsigned long long *>(snap->tracks);
            for (int w = tid; w < (int)(sizeof(sh.tab) / 8); w += kTrackThreads) dst[w] = src[w];
        }
        __syncthreads();
    }
    // the table, as the last frame left it (a launch whose frames were all refused leaves it untouched)
    if (advanced) {
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(sh.tab);
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(a.table->tracks);
        for (int w = tid; w < (int)(sizeof(sh.tab) / 8); w += kTrackThreads) dst[w] = src[w];
        if (tid == 0) { a.table->stamp = sh.stamp; a.table->stamped = sh.stamped; a.table->next_id = sh.next_id; }
    }
}

void launch_track_update(const TrackArgs &a, int batch, hipStream_t s)
{
    hipLaunchKernelGGL(track_kernel, dim3(1), dim3(kTrackThreads), 0, s, a, batch);
}

}   // namespace irmv
