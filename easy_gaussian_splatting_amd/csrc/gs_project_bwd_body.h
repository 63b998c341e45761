// The body of project_bwd_kernel / project_bwd_budget_kernel / project_bwd_depth_kernel / project_bwd_cm_kernel (gs_project.hip), which define DEG, ADAM,
// SUMS, the mask REG, the camera model CAM, the antialiased mode AA and SELECT (the fused form over the visible Gaussians only) around it.
// Included once per kernel template, inside its braces: no include guard, nothing but the body.
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (guard_tripped(a.guard)) return;
    if (ADAM && a.ad_applied != nullptr && blockIdx.x == 0 && threadIdx.x == 0) a.ad_applied[0] += 1;
    float* lds_cam = smem;
    int* vis_s = reinterpret_cast<int*>(smem + 32);
    float* tile = smem + 32 + kProjThreads;

    const int c = a.cam;
    const int64_t n0 = (int64_t)blockIdx.x * kProjThreads;
    const int64_t n = n0 + threadIdx.x;
    const int64_t f = (int64_t)c * a.N + n;
    const bool in_range = n < a.N;
    stage_camera(a.viewmats, a.Ks, c, a.W, a.H, lds_cam);   // (read after the row sum: read_camera)

    const bool vis = in_range && a.radii[f] > 0;
    const int cnt = vis ? a.tiles_per_gauss[f] : 0;
    const int base = vis ? a.cum_tiles[f] : 0;
    int r0 = 0, nr = 0;   // this Gaussian's gradient rows: [r0, r0 + nr)
    if (!SUMS && cnt > 0) { r0 = rows_before(a.row_base, a.qmask, base); nr = rows_before(a.row_base, a.qmask, base + cnt) - r0; }

    // ---- 1. sum this Gaussian's gradient rows (contiguous and compact, written once each by blend_bwd) -- or take the sums gs_row_sums
    //         left (a.row_sums: the view-parallel step forms them early, for the colour-gradient exchange)
    RowSum s;
    if (SUMS) {
        const float4* rs = reinterpret_cast<const float4*>(a.row_sums) + 3 * f;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x, z = x;
        if (vis) { x = rs[0]; y = rs[1]; z = rs[2]; }
        s.v[0] = x.x; s.v[1] = x.y; s.v[2] = x.z; s.v[3] = x.w; s.v[4] = y.x; s.v[5] = y.y; s.v[6] = y.z; s.v[7] = y.w;
        s.v[8] = z.x; s.v[9] = z.y; s.v[10] = z.z; s.v[11] = 0.f;
    } else {
        row_sum_wave(a, nr, r0, base, s, tile + (threadIdx.x >> 6) * kRowWaveFloats);
    }

    // ---- 2. colour path
    Camera cam;
    read_camera(lds_cam, cam);
    float v_mean[3] = {0.f, 0.f, 0.f}, v_quat[4] = {0.f, 0.f, 0.f, 0.f}, v_scale[3] = {0.f, 0.f, 0.f};
    float mean[3] = {0.f, 0.f, 0.f};
    // (the fused form reads its parameters through the flat buffer it updates: six pointers fewer to keep in SGPRs)
    const float* p_means = ADAM ? adam_p(a, 0) : a.means;
    const float* p_scales = ADAM ? adam_p(a, 1) : a.scales;
    const float* p_quats = ADAM ? adam_p(a, 2) : a.quats;
    const float* p_opac = ADAM ? adam_p(a, 5) : a.opacities;
    if (in_range) { mean[0] = p_means[3 * n]; mean[1] = p_means[3 * n + 1]; mean[2] = p_means[3 * n + 2]; }
    const float v_rgb[3] = {s.v[8], s.v[9], s.v[10]};
    if (DEG >= 0) {
        const int row_f = 3 * a.K, stride = row_f + 1;
        constexpr int ka3 = 3 * (DEG + 1) * (DEG + 1);
        // With the forward's direction Jacobian (a.sh_jac) the backward needs no SH coefficient: v_sh = Y (x) v_pre, and the
        // direction term of v_mean is J^T v_pre -- the block neither streams its 48 floats per Gaussian into LDS nor waits
        // for them (0.04 ms of the fused step kernel; the forward pays 36 B per visible Gaussian and ~200 FMAs).
        const bool use_jac = a.sh_jac != nullptr;
        float G[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float rgb[3] = {0.f, 0.f, 0.f};
        if (vis) {   // (requested before the barrier)
            rgb[0] = a.colors_post[3 * f]; rgb[1] = a.colors_post[3 * f + 1]; rgb[2] = a.colors_post[3 * f + 2];
            if (use_jac && DEG >= 1) {
                const float4 j0 = a.sh_jac[2 * f], j1 = a.sh_jac[2 * f + 1];
                G[10] = reinterpret_cast<const float*>(a.sh_jac + 2 * (int64_t)a.C * a.N)[f];
                G[0] = j0.x; G[1] = j0.y; G[2] = j0.z; G[4] = j0.w; G[5] = j1.x; G[6] = j1.y; G[8] = j1.z; G[9] = j1.w;
            }
        }
        vis_s[threadIdx.x] = vis ? 1 : 0;
        __syncthreads();   // (every wave is done with its row-sum scratch in `tile`)
        if (SELECT) {
            // Nobody in the block was seen: no parameter of it moves.  What the dense kernel leaves behind for culled Gaussians is the
            // absgrad side channel alone (the fused entry hands out no other per-Gaussian output) -- no SH staging, no Adam walk.
            const int l = threadIdx.x & 63;
            static_assert(kProjThreads == 256, "the block-wide OR below reads four flags per lane");
            if (__ballot(vis_s[l] | vis_s[l + 64] | vis_s[l + 128] | vis_s[l + 192]) == 0) {
                if (in_range) reinterpret_cast<float2*>(a.v_means2d_abs)[f] = make_float2(s.v[2], s.v[3]);
                return;
            }
        }
        const int rows = (int)min((int64_t)kProjThreads, a.N - n0);
        if (!use_jac) {
            if (a.sh_rest) {
                if (DEG == 4) stage_sh_rows_split<25>(a.colors_in, a.sh_rest, n0, rows, 25, ka3, vis_s, tile);   // (SH4: K = 25)
                else if (a.K == 16) stage_sh_rows_split<16>(a.colors_in, a.sh_rest, n0, rows, 16, ka3, vis_s, tile);
                else stage_sh_rows_split<0>(a.colors_in, a.sh_rest, n0, rows, a.K, ka3, vis_s, tile);
            } else {
                if (DEG == 4) stage_sh_rows<25>(a.colors_in, n0, rows, 25, ka3, vis_s, tile);
                else if (a.K == 16) stage_sh_rows<16>(a.colors_in, n0, rows, 16, ka3, vis_s, tile);
                else stage_sh_rows<0>(a.colors_in, n0, rows, a.K, ka3, vis_s, tile);
            }
            __syncthreads();
        }
        float* my = tile + threadIdx.x * stride;
        if (vis) {
            float ux, uy, uz;
            const float dn = view_dir(mean, cam, ux, uy, uz);
            if (use_jac) sh_vjp_jac(DEG < 0 ? 0 : DEG, G, rgb, v_rgb, ux, uy, uz, dn, my, v_mean);
            else sh_vjp(DEG < 0 ? 0 : DEG, my, rgb, v_rgb, ux, uy, uz, dn, my, v_mean, false);
            for (int o = ka3; o < row_f; ++o) my[o] = 0.f;
            if (a.v_colors_pre) {  // gradient w.r.t. the pre-clamp colour: what gs_sh_grad_views consumes
                float* d = a.v_colors_pre + 3 * f;
                d[0] = rgb[0] > 0.f ? v_rgb[0] : 0.f; d[1] = rgb[1] > 0.f ? v_rgb[1] : 0.f; d[2] = rgb[2] > 0.f ? v_rgb[2] : 0.f;
            }
        } else if (in_range) {
            for (int o = 0; o < row_f; ++o) my[o] = 0.f;
            if (a.v_colors_pre) { float* d = a.v_colors_pre + 3 * f; d[0] = 0.f; d[1] = 0.f; d[2] = 0.f; }
        }
        if (ADAM) {
            __syncthreads();
            if (DEG == 4) adam_sh_tile<25, SELECT>(tile, rows, 25, n0, a, vis_s);
            else if (a.K == 16) adam_sh_tile<16, SELECT>(tile, rows, 16, n0, a, vis_s);
            else adam_sh_tile<0, SELECT>(tile, rows, a.K, n0, a, vis_s);
        } else if (a.v_colors) {  // NULL: the caller rebuilds the SH gradients from v_colors_pre (gs_sh_grad_views)
            __syncthreads();
            if (DEG == 4) write_sh_tile_k<25>(tile, rows, 25, n0, a.v_colors, a.v_sh_rest, a.accumulate);
            else write_sh_tile(tile, rows, a.K, n0, a.v_colors, a.v_sh_rest, a.accumulate);
        }
    } else if (in_range) {
        if (a.colors_per_camera) {
            float* d = a.v_colors + 3 * f;
            d[0] = v_rgb[0]; d[1] = v_rgb[1]; d[2] = v_rgb[2];
        } else {
            float* d = a.v_colors + 3 * n;
            if (a.accumulate) { d[0] += v_rgb[0]; d[1] += v_rgb[1]; d[2] += v_rgb[2]; }
            else { d[0] = v_rgb[0]; d[1] = v_rgb[1]; d[2] = v_rgb[2]; }
        }
    }

    // ---- 3. projection VJP
    float sc_fac[3] = {1.f, 1.f, 1.f}, op_fac = 1.f;   // d activated / d raw (identity without activations)
    float aa_vop = 0.f;   // (AA) the activated opacity's gradient: the record opacity's (s.v[7]) times d record / d activated = the chain's rho
    if (vis) {
        const float4 q4 = reinterpret_cast<const float4*>(p_quats)[n];
        const float quat[4] = {q4.x, q4.y, q4.z, q4.w};
        const float scale[3] = {act_scale(p_scales[3 * n], a.activations), act_scale(p_scales[3 * n + 1], a.activations),
                                act_scale(p_scales[3 * n + 2], a.activations)};
        if (a.activations) { sc_fac[0] = scale[0]; sc_fac[1] = scale[1]; sc_fac[2] = scale[2]; }
        ProjChainT<preal> p;
        // (AA) s.v[7] is the gradient of the record's opacity, opacity * rho: times the opacity it reaches rho and through it cov2_0
        if (project_chain<preal, CAM, AA>(mean, quat, scale, cam, a.eps2d, a.near_p, a.far_p, p)) {
            preal v_rho = 0;
            if (AA) v_rho = (preal)s.v[7] * (preal)act_opacity(p_opac[n], a.activations);
            project_vjp<preal, CAM, AA>(scale, cam, p, s.v[0], s.v[1], s.v[4], s.v[5], s.v[6], 0.f, v_mean, v_quat, v_scale, v_rho, (preal)a.eps2d);
            if (AA) {
                if (!ADAM && a.v_op_rec) a.v_op_rec[f] = s.v[7];   // (gs_project_bwd_cam_aa: the camera kernel forms v_rho from it)
                aa_vop = s.v[7] * (float)p.rho;
            }
        }
    }
    if ((REG & 4) && in_range) {   // + the depth channel's gradient (culled Gaussians: v_z = 0), onto the rounded v_mean as gs_depth_grads adds it
        const float row2[3] = {lds_cam[6], lds_cam[7], lds_cam[8]};   // (make_camera: R[6..8] = row 2 of the view matrix, as it lies there)
        v_mean[0] = fp_opaque(v_mean[0]); v_mean[1] = fp_opaque(v_mean[1]); v_mean[2] = fp_opaque(v_mean[2]);
        depth_vjp_mean(a.v_depths[f], row2, v_mean);
    }
    float geo_op = 0.f;
    if (in_range) {
        if (a.activations && vis) { const float o = act_opacity(p_opac[n], 1); op_fac = o * (1.f - o); }
        v_scale[0] *= sc_fac[0]; v_scale[1] *= sc_fac[1]; v_scale[2] *= sc_fac[2];
        // + the regulariser's gradient (culled Gaussians too: every Gaussian has a term), from the parameters before the update
        // (SELECT: a culled Gaussian's term is not formed -- nothing reads it)
        if ((REG & 1) && (!SELECT || vis)) {
            float gl[3];
            scale_reg_term(p_scales[3 * n], p_scales[3 * n + 1], p_scales[3 * n + 2], a.reg_ratio, a.reg_grad, gl);
            v_scale[0] = fp_opaque(v_scale[0]) + gl[0]; v_scale[1] = fp_opaque(v_scale[1]) + gl[1]; v_scale[2] = fp_opaque(v_scale[2]) + gl[2];
        }
        float v_op = s.v[7] * op_fac;
        if (AA) v_op = aa_vop * op_fac;
        if (REG & 2) {   // + the budget regulariser's gradients, as gs_mcmc_reg adds them to the gradients gs_project_bwd wrote
            double o, sk[3];
            float go, gl[3];
            budget_reg_term(p_opac[n], p_scales[3 * n], p_scales[3 * n + 1], p_scales[3 * n + 2], a.bud_ga, a.bud_gb, &o, sk, &go, gl);
            v_scale[0] = fp_opaque(v_scale[0]) + gl[0]; v_scale[1] = fp_opaque(v_scale[1]) + gl[1]; v_scale[2] = fp_opaque(v_scale[2]) + gl[2];
            v_op = fp_opaque(v_op) + go;
        }
        float* vm = a.v_means + 3 * n; float* vq = a.v_quats + 4 * n; float* vs = a.v_scales + 3 * n;
        if (ADAM) {
            geo_op = v_op;   // (applied block-wide below: adam_geo_tile)
            if (a.st_max_radii != nullptr && vis) {   // same arithmetic as update_statistics_kernel
                a.st_max_radii[n] = fmaxf(a.st_max_radii[n], (float)a.radii[f] * (1.f / a.st_max_hw));
                a.st_grad_norm[n] += sqrtf(s.v[2] * s.v[2] + s.v[3] * s.v[3]) * a.st_max_hw;
                a.st_counts[n] += 1.f;
            }
        } else if (a.accumulate) {
            vm[0] += v_mean[0]; vm[1] += v_mean[1]; vm[2] += v_mean[2];
            vq[0] += v_quat[0]; vq[1] += v_quat[1]; vq[2] += v_quat[2]; vq[3] += v_quat[3];
            vs[0] += v_scale[0]; vs[1] += v_scale[1]; vs[2] += v_scale[2];
            a.v_opacities[n] += v_op;
        } else {
            vm[0] = v_mean[0]; vm[1] = v_mean[1]; vm[2] = v_mean[2];
            vq[0] = v_quat[0]; vq[1] = v_quat[1]; vq[2] = v_quat[2]; vq[3] = v_quat[3];
            vs[0] = v_scale[0]; vs[1] = v_scale[1]; vs[2] = v_scale[2];
            a.v_opacities[n] = v_op;
        }
        reinterpret_cast<float2*>(a.v_means2d_abs)[f] = make_float2(s.v[2], s.v[3]);
        if (SUMS && a.st_gn_out) {   // (only with row_sums: the view-parallel step; the row-walking form keeps HEAD's registers)
            a.st_gn_out[n] = vis ? sqrtf(s.v[2] * s.v[2] + s.v[3] * s.v[3]) * a.st_max_hw : 0.f;   // (update_statistics_kernel's arithmetic)
            a.st_cnt_out[n] = vis ? 1.f : 0.f;
        }
        if (a.v_means2d) reinterpret_cast<float2*>(a.v_means2d)[f] = make_float2(s.v[0], s.v[1]);
        if (a.v_conics) { a.v_conics[3 * f] = s.v[4]; a.v_conics[3 * f + 1] = s.v[5]; a.v_conics[3 * f + 2] = s.v[6]; }
        if (a.v_colors_post) { a.v_colors_post[3 * f] = v_rgb[0]; a.v_colors_post[3 * f + 1] = v_rgb[1]; a.v_colors_post[3 * f + 2] = v_rgb[2]; }
    }
    if (DEG >= 0 && ADAM) {
        // Geometry Adam, block-wide: the 11 gradients of every Gaussian of the block go through LDS into element order, and
        // means / log-scales / quaternions / logit-opacities (+ their moments) are updated with 16-byte accesses, every load
        // of a thread issued before its first store.  One gradient per thread and launch-order scalar accesses (33 dependent
        // load -> store round trips per thread: the in-place stores may alias the next loads as far as the compiler can
        // tell) took 0.08 ms of the step for 0.3 GB; same arithmetic per element, bit-identical update.
        __syncthreads();   // (adam_sh_tile is done with the tile; every thread has read its own parameters)
        float* gm = tile;
        float* gs = tile + 3 * kProjThreads;
        float* gq = tile + 6 * kProjThreads;
        float* go = tile + 10 * kProjThreads;
        const int tid = threadIdx.x;
        gm[3 * tid] = v_mean[0]; gm[3 * tid + 1] = v_mean[1]; gm[3 * tid + 2] = v_mean[2];
        gs[3 * tid] = v_scale[0]; gs[3 * tid + 1] = v_scale[1]; gs[3 * tid + 2] = v_scale[2];
        gq[4 * tid] = v_quat[0]; gq[4 * tid + 1] = v_quat[1]; gq[4 * tid + 2] = v_quat[2]; gq[4 * tid + 3] = v_quat[3];
        go[tid] = geo_op;
        __syncthreads();
        adam_geo_tile<SELECT>(tile, (int)min((int64_t)kProjThreads, a.N - n0), n0, a, vis_s);
    }
