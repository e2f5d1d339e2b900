// The walk of net_fused_tc8_kernel for one launch (fused.hip includes this text twice: as the kernel's body and as net_fused_tc8_walk's).
// It expects in the enclosing scope: the template parameters NW (waves), T0 (frames), WD (< 0: the round-2 layers), NTJ0 (the arm of the
// nine-tap layers, below), TM (time-major plan) and IMG (weights from the frozen table's image) as compile-time constants, and the kernel
// arguments `const FusedArgs& a` (or by value).  It defines and undefines TCR_TC8, TCR_TC8_R, TCR_TC8_OCS, TCR_TC8_WIO and TCR_TC8_BARRIER;
// the order of its TCR_TC8 / TCR_TC8_R calls is the order of tc8_shape's rows (fused.hip), which also fixes the image's layer order.
    constexpr int NT = NW * 64;
    constexpr int T1 = (T0 + 1) / 2, T2 = (T1 + 1) / 2;
    float* lds = reinterpret_cast<float*>(dyn_lds());
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int row = a.in_c * a.in_tp;
#if TCR_FUSED_WHATIF & 2048
    // phase timing (diagnostic side build, WRONG outputs): cycles between the barriers, written over the group's first probabilities
    long long ts[14];
    int nts = 0;
#define TCR_TC8_BARRIER do { __syncthreads(); ts[nts++] = (long long)__builtin_readcyclecounter(); } while (0)
#elif TCR_FUSED_WHATIF & 8
#define TCR_TC8_BARRIER ((void)0)
#else
#define TCR_TC8_BARRIER __syncthreads()
#endif
    // (Measured and removed, round 6: the upper half of the waves running a block's first conv BEFORE its shortcut conv -- both read the same rows --
    //  so that a SIMD's two waves are not in the shortcut's load / store-bound jobs together: 96.5 vs 95.6 us at 49 frames, 173.9 vs 176.1 at 98.)
    // (tiles per job: two; NTJ0 = 4: four for block 0's layers -- 16 / 24 channels at T0 / 2 frames --, the TCR_TUNE_NET_FUSED = 5 arm)
    // (NTJ0 = 0: the nine-tap layers' work dealt in 16-position units, fused_layer_u)
    // (NTJ0 = 6: conv0_1 -- block 0's nine-tap layer of 24 input channels -- in its resident-weight form, fused_layer_r; every other layer as NTJ0 = 3)
    // (Measured and removed: conv1_0 -- block 1's stride-2 nine-tap layer, 24 -> 32 -- resident too in the time-major plan, its set requested in front of the
    //  barrier behind conv0_1, each tile's live taps walked behind a uniform test per tap, the shortcut conv behind it: 71.1 us against 69.6, its phase 20.6 ->
    //  22.7 k cycles; the no-refill what-if had predicted 69.5 us: OPTLOG "fragment-ordered frozen weights")
    constexpr bool RES = WD >= 0 && NTJ0 == 6;
    constexpr int NTJU = RES ? 3 : NTJ0;
    // (who reads layer LI's output rows: nobody convolves a shortcut conv's or the last layer's; a block's first conv feeds its stride-1 second, which feeds the next block's stride-2 layers)
#define TCR_TC8_OCS(LI, K_, S_) ((K_ == 1 || LI == 9) ? 0 : (S_ == 2 ? 1 : 2))
    // (IMG: where layer LI's fragments start in the image -- the layers' images follow one another)
#define TCR_TC8_WIO(LI) (IMG ? tc8_wimg_off(LI) : 0)
#define TCR_TC8(LI, K_, S_, CI_, CO_, T_) do { const FusedLayer& L_ = TCR_LAYER_ROW(WD >= 0, LI); \
        static_assert(tc8_shape(LI).k == K_ && tc8_shape(LI).stride == S_ && tc8_shape(LI).cin == CI_ && tc8_shape(LI).cout == CO_, "layer LI runs with row LI's shape (tc8_shape)"); \
        if constexpr (TM) fused_layer_tm<NW, K_, S_, CI_, CO_, T_, (LI == 3 || LI == 6 || LI == 9), TCR_TC8_OCS(LI, K_, S_), ((K_ == 9 && CI_ <= 32) ? 1 : 0), IMG>(a, L_, lds, ng, wave, r, q, TCR_TC8_WIO(LI)); \
        else fused_layer_sel<NW, K_, S_, CI_, CO_, T_, WD, (LI == 3 || LI == 6 || LI == 9), (K_ != 1 && LI != 9), ((LI >= 1 && LI <= 3 && NTJU == 4) ? 4 : (((NTJU == 0 || NTJU == 3) && K_ == 9) ? NTJU : 2))>(a, L_, lds + a.buf_off[L_.in_buf], L_.in_sz, lds, ng, wave, r, q); } while (0)
    // (resident form of layer LI: halo zeros of its output rows, then the walk out of the set WS_ requested in front of the barrier)
#define TCR_TC8_R(LI, S_, CI_, CO_, T_, WS_) do { const FusedLayer& L_ = TCR_LAYER_ROW(true, LI); \
        if constexpr (TM) fused_zero_halo_tm<NT, CO_, (T_ + S_ - 1) / S_, fused_tm_pitch((T_ + S_ - 1) / S_, true, TCR_TC8_OCS(LI, 9, S_))>(lds + a.buf_off[L_.out_buf], tid); \
        else fused_zero_halo<NT, CO_, (T_ + S_ - 1) / S_>(lds + a.buf_off[L_.out_buf], L_.out_sz, ng, tid); \
        fused_layer_r<NW, 9, S_, CI_, CO_, T_, (LI == 3), TM, TCR_TC8_OCS(LI, 9, S_), IMG>(a, L_, lds + a.buf_off[L_.in_buf], L_.in_sz, lds, ng, wave, r, q, WS_); } while (0)
    for (int grp = blockIdx.x; grp < (TCR_WHATIF(512) ? 0 : a.n_groups); grp += gridDim.x) {
        const int n0 = grp * a.group;
        const int ng = min(a.group, a.batch - n0);
#if TCR_FUSED_WHATIF & 2048
        nts = 0;
        ts[nts++] = (long long)__builtin_readcyclecounter();
#endif
        if constexpr (WD < 0) fused_layer_sel<NW, 3, 1, 40, 16, T0, WD, false>(a, a.layer[0], a.feat + (size_t)n0 * row, row, lds, ng, wave, r, q);
        else if (!TCR_WHATIF(64)) {
            const FusedLayer& L0 = TCR_LAYER_ROW(true, 0);
            if constexpr (TM) {
                fused_zero_halo_tm<NT, 16, T0, fused_tm_pitch(T0, true, 2)>(lds + a.buf_off[L0.out_buf], tid);
                fused_conv0_s<NW, T0, false, TCR_TM_CONV0, IMG>(a, L0, a.feat + (size_t)n0 * row, row, lds, ng, wave, r, q, 0, TCR_TC8_WIO(0));
            } else {
            fused_zero_halo<NT, 16, T0>(lds + a.buf_off[L0.out_buf], L0.out_sz, ng, tid);
            fused_conv0_s<NW, T0>(a, L0, a.feat + (size_t)n0 * row, row, lds, ng, wave, r, q);
            }
        }
        if constexpr (RES) {
            float ws3[9 * 6];
            TCR_TC8_BARRIER;
            TCR_TC8(1, 1, 2, 16, 24, T0);
            TCR_TC8(2, 9, 2, 16, 24, T0);
            fused_resident_request<NW, 9, 24, 24, IMG>(a, TCR_LAYER_ROW(true, 3), wave, r, q, ws3, TCR_TC8_WIO(3));      // (no job state is live here: the set costs no register of the budget)
            TCR_TC8_BARRIER;
            TCR_TC8_R(3, 1, 24, 24, T1, ws3);
            TCR_TC8_BARRIER;
        } else {
        TCR_TC8_BARRIER;
        TCR_TC8(1, 1, 2, 16, 24, T0);           // block0/down (reads the same rows as conv0_0: no barrier in between)
        TCR_TC8(2, 9, 2, 16, 24, T0);
        TCR_TC8_BARRIER;
        TCR_TC8(3, 9, 1, 24, 24, T1);
        TCR_TC8_BARRIER;
        }
        TCR_TC8(4, 1, 2, 24, 32, T1);
        TCR_TC8(5, 9, 2, 24, 32, T1);
        TCR_TC8_BARRIER;
        TCR_TC8(6, 9, 1, 32, 32, T2);
        TCR_TC8_BARRIER;
        TCR_TC8(7, 1, 2, 32, 48, T2);
        TCR_TC8(8, 9, 2, 32, 48, T2);
        TCR_TC8_BARRIER;
        TCR_TC8(9, 9, 1, 48, 48, (T2 + 1) / 2);
        TCR_TC8_BARRIER;
        if constexpr (WD < 0) fused_head<NT>(a, lds, n0, ng, tid);
        else if (!TCR_WHATIF(16)) {
            if (a.nc == 12 || TM) fused_head_s<NT, 48, (T2 + 1) / 2, 12, TM>(a, lds, n0, ng, tid);      // (time-major: launched for 12 classes only)
            else fused_head<NT>(a, lds, n0, ng, tid);
        }
#if TCR_FUSED_WHATIF & 2048
        __syncthreads();
        ts[nts++] = (long long)__builtin_readcyclecounter();
        if (tid == 0)
            for (int i = 0; i + 1 < nts && i < 12; ++i) a.probs[(size_t)n0 * a.nc + i] = (float)(ts[i + 1] - ts[i]);
#endif
    }
#undef TCR_TC8
#undef TCR_TC8_WIO
#undef TCR_TC8_OCS
#undef TCR_TC8_R
#undef TCR_TC8_BARRIER
