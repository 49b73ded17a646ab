// The body of stem_pool_bf16s_kernel<MODE> (stem_bf16s.h), included once per patch SOURCE: as it stands it stages the normalised fp32 planar frames
// (`left`, `right`); with STEM_SRC_U8 defined it stages the camera's bytes (`left8`, `right8`: uint8 [B, HIN, HIN, 3]; `table` fp32 [3][256]) and MODE is 0.
// A textual include on purpose: the fp32-source kernels are token for token what they were before the byte source existed, so their code objects are too.
    using Cfg = StemPoolCfg;
    constexpr int R = Cfg::R, SR = Cfg::SR, PR = Cfg::PR, XS = Cfg::XS, PCOLS = Cfg::PCOLS, PITCH = Cfg::PITCH, THREADS = Cfg::THREADS, NPRE = Cfg::NPRE;
    extern __shared__ __attribute__((aligned(16))) char sp_sm[];
    char* patch = sp_sm;
    char* ring = sp_sm + Cfg::OFF_RING;
    char* carry = sp_sm + Cfg::OFF_CARRY;
    float* bn_sc = (float*)(sp_sm + Cfg::OFF_BN);
    float* bn_sh = bn_sc + 128;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, xl = lane & 31, h = lane >> 5;
    const int HO = HIN / 2, HP = HIN / 4, xsegs = HO / XS, groups = HP / R;
    // a workgroup takes whole (image, row group) runs -- run blockIdx.x + k gridDim.x -- and walks a run's segments left to right, so a
    // carried column always comes from the item it processed just before; q = position in that sequence
    const long runs = (long)nimg * groups;
    const long my_runs = (long)blockIdx.x < runs ? (runs - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    const long nq = my_runs * xsegs;
    auto decode = [&](long q, int& seg, int& g, int& n) __attribute__((always_inline)) {
        const long run = blockIdx.x + (q / xsegs) * (long)gridDim.x;
        seg = (int)(q % xsegs);
        g = (int)(run % groups);
        n = (int)(run / groups);
    };

    if (MODE == 0 && tid < 64) {
        const float sc = gamma[tid] / sqrtf(var[tid] + 1e-5f);
        bn_sc[tid] = sc;
        bn_sh[tid] = beta[tid] - mean[tid] * sc;
    }
    if (MODE == 2 && tid < 128) { bn_sc[tid] = gamma[tid]; bn_sh[tid] = beta[tid]; }
#ifdef STEM_SRC_U8
    for (int i = tid; i < 3 * 256; i += THREADS) ((__bf16*)(sp_sm + Cfg::LDS_BYTES))[i] = (__bf16)table[i];      // the value table as bf16, behind the BatchNorm tables
#endif
    f32x16 ssum[2], ssq[2];                                  // MODE 1 only (dead otherwise)
#pragma unroll
    for (int r = 0; r < 16; ++r) { ssum[0][r] = 0.f; ssum[1][r] = 0.f; ssq[0][r] = 0.f; ssq[1][r] = 0.f; }
    // ---- A fragments: channel mt * 32 + xl, k row rr = 2 step + h (c = rr / 7, ky = rr % 7), element j = kx (7 -> zero)
    bf16x8 af[2][11];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int st = 0; st < 11; ++st) {
            const int rr = 2 * st + h;
            const float* wp = w + (mt * 32 + xl) * 147 + rr * 7;       // rr * 7 = c * 49 + ky * 7
#pragma unroll
            for (int j = 0; j < 8; ++j) af[mt][st][j] = (__bf16)((j < 7 && rr < 21) ? wp[j] : 0.f);
        }
    // byte offset of this lane's (c, ky) row per step inside the patch (the padded row 21 reads row 20: its weights are zero)
    int roff[11];
#pragma unroll
    for (int st = 0; st < 11; ++st) {
        const int rr = min(2 * st + h, 20);
        roff[st] = ((rr / 7) * PR + rr % 7) * PITCH;
    }

    // ---- patch staging: pair i = tid + j * THREADS -> (channel, patch row, column pair); patch row pr <-> input row 4 py0 - 5 + pr,
    // patch column pc <-> input column 2 c0 - 3 + pc (c0 = first stem column of the segment)
    auto stage = [&](int seg, int g, int n) __attribute__((always_inline)) {
#ifdef STEM_SRC_U8
        constexpr int NG = StemPoolU8::NG, ITEMS = PR * NG, NIT = (ITEMS + THREADS - 1) / THREADS;       // 1365 groups, 6 per thread
        static_assert(4 * NG - 1 >= Cfg::PCOLS && NIT % 3 == 0, "the groups cover the patch columns; chunks of three");
        const unsigned char* src = ((n & 1) ? right8 : left8) + (long)(n >> 1) * 3 * HIN * HIN;
        const unsigned short* tb = (const unsigned short*)(sp_sm + Cfg::LDS_BYTES);
        const int iy0 = 4 * g * R - 5, gx0 = 2 * seg * XS - 4;
#pragma unroll 1
        for (int j0 = 0; j0 < NIT; j0 += 3) {
            unsigned raw[3][3];
            int dst[3], gg_[3];
            bool ok[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i = tid + (j0 + j) * THREADS;
                const int pr = i / NG, gg = i - pr * NG;
                const int y = iy0 + pr, x = gx0 + 4 * gg;
                ok[j] = i < ITEMS && y >= 0 && y < HIN && x >= 0 && x + 3 < HIN;
                const unsigned* rp = (const unsigned*)(src + ((long)y * HIN + x) * 3);
#pragma unroll
                for (int k = 0; k < 3; ++k) raw[j][k] = ok[j] ? rp[k] : 0u;
                dst[j] = pr * PITCH + (4 * gg - 1) * 2;                        // (-2 for row 0, group 0: its first pixel is never written)
                gg_[j] = i < ITEMS ? gg : -1;
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (gg_[j] < 0) continue;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    unsigned v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int bi = 3 * e + c;                               // byte of (pixel e, channel c) inside the 12
                        const unsigned b = (raw[j][bi >> 2] >> (8 * (bi & 3))) & 255u;
                        v[e] = ok[j] ? (unsigned)tb[c * 256 + b] : 0u;
                    }
                    char* p = patch + c * PR * PITCH + dst[j];
                    if (gg_[j] > 0) *(unsigned short*)p = (unsigned short)v[0];                     // group 0's first pixel is left of the patch
                    if (gg_[j] < NG - 1) {                                                          // the last group: only its first pixel is a patch column
                        *(unsigned*)(p + 2) = v[1] | (v[2] << 16);
                        *(unsigned short*)(p + 6) = (unsigned short)v[3];
                    }
                }
            }
        }
#else
        const float* src = ((n & 1) ? right : left) + (long)(n >> 1) * 3 * HIN * HIN;
        const int iy0 = 4 * g * R - 5, ix0 = 2 * seg * XS - 3;
        // chunks of 8 column pairs per thread: 16 loads in flight, then convert and write (the index arithmetic is redone per chunk on
        // purpose: hoisted out of the segment loop it would hold 100+ registers next to the 88 of the weights)
#pragma unroll 1
        for (int j0 = 0; j0 < NPRE; j0 += 8) {
            float pre[8][2];
            int dst[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = tid + (j0 + j) * THREADS;
                const int c = i / (PR * (PCOLS / 2)), rem = i - c * (PR * (PCOLS / 2)), pr = rem / (PCOLS / 2), pp = rem - pr * (PCOLS / 2);
                const int y = iy0 + pr, x = ix0 + 2 * pp;
                const bool rowok = c < 3 && y >= 0 && y < HIN;
                const float* rp = src + ((long)c * HIN + y) * HIN;
                pre[j][0] = (rowok && x >= 0 && x < HIN) ? rp[x] : 0.f;
                pre[j][1] = (rowok && x + 1 >= 0 && x + 1 < HIN) ? rp[x + 1] : 0.f;
                dst[j] = c < 3 ? (c * PR + pr) * PITCH + pp * 4 : -1;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                typedef __bf16 bf16x2s __attribute__((ext_vector_type(2)));
                bf16x2s v;
                v[0] = (__bf16)pre[j][0];
                v[1] = (__bf16)pre[j][1];
                if (dst[j] >= 0) *(bf16x2s*)(patch + dst[j]) = v;
            }
        }
#endif
    };

    const int t = wid & 1, par = wid >> 1;                   // 32-pixel tile of the segment, row of the pair
    const int pcol = 1 + 32 * t + xl;                        // ring column of this lane's pixel (column 0 = the pixel left of the segment)
    const int key = (pcol & 7) << 1;                         // 8-byte chunk swizzle of a ring pixel: chunk ch sits at ch ^ key (pairs stay in order)
    // pooling duty: pooled column ppx, channels 8 u .. 8 u + 7
    const int ppx = tid >> 3, u = tid & 7;

    int cbuf = 0;                                            // carry buffer the current segment READS (its left neighbour's last column)
    for (long q = 0; q < nq; ++q) {
        int seg, g, n;
        decode(q, seg, g, n);
        __syncthreads();                                     // the previous segment's MFMAs and pooling are done with patch and ring
        stage(seg, g, n);
        __syncthreads();
        const int py0 = g * R;
        for (int pair = 0; pair <= R; ++pair) {
            const int ys = 2 * pair - 1 + par;               // stem row 2 py0 - 1 + ys; pair 0: only ys = 0 (waves 2-3)
            const int ystem = 2 * py0 - 1 + ys;
            f32x16 acc[2];
            const bool rowact = ys >= 0;
            if (rowact) {
#pragma unroll
                for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
                const char* bp = patch + (2 * ys) * PITCH + (32 * t + xl) * 4;
#pragma unroll
                for (int st = 0; st < 11; ++st) {
                    const unsigned* q = (const unsigned*)(bp + roff[st]);
                    u32x4s raw = {q[0], q[1], q[2], q[3]};
                    const bf16x8 bfrag = __builtin_bit_cast(bf16x8, raw);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][st], bfrag, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][st], bfrag, acc[1], 0, 0, 0);
                }
            }
            if constexpr (MODE == 1) {
                if (ys >= 1) {
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) { ssum[mt][r] += acc[mt][r]; ssq[mt][r] += acc[mt][r] * acc[mt][r]; }
                }
                continue;
            }
            const int eo = MODE == 2 ? (n & 1) * 64 : 0;      // this run's eye selects the scale / shift table
            __syncthreads();                                 // A: the previous pair's pooling has read its three ring rows
            if (rowact) {
                char* rrow = ring + (ys & 3) * Cfg::RING_ROW;
                const bool zero_row = ystem < 0;             // the row above the image: max-pool padding
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        const int co0 = mt * 32 + 8 * gq + 4 * h;
                        const f32x4 sc = *(const f32x4*)(bn_sc + eo + co0), sh = *(const f32x4*)(bn_sh + eo + co0);
                        bf16x4s o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float v = fmaxf(acc[mt][4 * gq + e] * sc[e] + sh[e], 0.f);
                            o[e] = (__bf16)(zero_row ? 0.f : v);
                        }
                        const int ch = co0 >> 2;
                        *(bf16x4s*)(rrow + pcol * 128 + ((ch ^ key) << 3)) = o;
                        if (t == 1 && xl == 31) *(bf16x4s*)(carry + ((cbuf ^ 1) * SR + ys) * 128 + (ch << 3)) = o;       // last column: the next segment's left neighbour
                    }
                if (t == 0 && lane < 16) {                   // ring column 0: zero (image edge) or the carried column of the previous segment
                    bf16x4s c0v = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
                    if (seg > 0) c0v = *(const bf16x4s*)(carry + (cbuf * SR + ys) * 128 + (lane << 3));
                    *(bf16x4s*)(rrow + (lane << 3)) = c0v;  // key(0) = 0
                }
            }
            __syncthreads();                                 // B: both rows of the pair are in the ring
            if (pair >= 1) {
                // pooled row py0 + pair - 1 from stem rows ys = 2 pair - 2, 2 pair - 1, 2 pair; pooled column ppx from ring columns 2 ppx .. 2 ppx + 2
                u16x8s m = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const char* rrow = ring + ((2 * pair - 2 + dy) & 3) * Cfg::RING_ROW;
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int pc = 2 * ppx + dx;
                        const u16x8s v = *(const u16x8s*)(rrow + pc * 128 + (((2 * u) ^ ((pc & 7) << 1)) << 3));
                        m = __builtin_elementwise_max(m, v);
                    }
                }
                const long prow = ((long)(n >> 1) * HP + py0 + pair - 1) * HP + seg * (XS / 2) + ppx;
                *(u16x8s*)((char*)out + (prow * 128 + (n & 1) * 64 + u * 8) * 2) = m;
            }
        }
        cbuf ^= 1;                                           // the column this segment saved is the next segment's neighbour
    }
    if constexpr (MODE == 1) {
        // lanes of equal h hold the same 32 channels for 32 pixel columns: fold the 32 columns (fixed order), then the four waves through LDS
        __syncthreads();
        float* red = (float*)sp_sm;                          // [wave][64 channels][2]
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float a = ssum[mt][r], b = ssq[mt][r];
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
                if (xl == 0) {
                    const int co = mt * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
                    red[(wid * 64 + co) * 2] = a;
                    red[(wid * 64 + co) * 2 + 1] = b;
                }
            }
        __syncthreads();
        if (tid < 128) {
            const int co = tid >> 1, qq = tid & 1;
            const float a = (nq > 0) ? red[(0 * 64 + co) * 2 + qq] + red[(1 * 64 + co) * 2 + qq] + red[(2 * 64 + co) * 2 + qq] + red[(3 * 64 + co) * 2 + qq] : 0.f;
            const int groups_ = HP / R;
            const int eye = (int)((blockIdx.x / groups_) & 1);
            float* part = (float*)out + (long)blockIdx.x * 256;
            part[(eye * 64 + co) * 2 + qq] = a;
            part[((eye ^ 1) * 64 + co) * 2 + qq] = 0.f;
        }
    }
