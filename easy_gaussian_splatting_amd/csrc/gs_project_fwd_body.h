// The body of project_fwd_kernel / project_fwd_cm_kernel (gs_project.hip), which define DEG, STAGE, the camera model CAM and
// the antialiased mode AA around it.
// Included once per kernel template, inside its braces: no include guard, nothing but the body.
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* lds_cam = smem;
    int* vis_s = reinterpret_cast<int*>(smem + 32);
    float* tile = smem + 32 + kProjThreads;

    const int c = blockIdx.y;
    const int64_t n0 = (int64_t)blockIdx.x * kProjThreads;
    const int64_t n = n0 + threadIdx.x;
    const int64_t f = (int64_t)c * a.N + n;
    const bool in_range = n < a.N;
    Camera cam;
    load_camera(a.viewmats, a.Ks, c, a.W, a.H, lds_cam, cam);

    // one-launch forward, full SH3 rows in the split layout (what the reference model trains with): the block's SH slice is
    // requested now and consumed after the projection chain (sh_rows_issue)
    const bool prefetch_sh = STAGE == 0 && DEG == 3 && a.sh_rest != nullptr && a.K == 16 && (((uintptr_t)a.sh_rest & 15) == 0);
    // (vector memory loads return in issue order: the geometry inputs are requested FIRST, so that the chain below waits
    //  for them only and runs while the SH slice is still in flight)
    float mean[3] = {0.f, 0.f, 0.f};
    if (in_range) { mean[0] = a.means[3 * n]; mean[1] = a.means[3 * n + 1]; mean[2] = a.means[3 * n + 2]; }
    float4 q4 = make_float4(1.f, 0.f, 0.f, 0.f);
    float sc_raw[3] = {0.f, 0.f, 0.f}, op_raw = 0.f;
    if (STAGE != 2 && in_range) {
        q4 = reinterpret_cast<const float4*>(a.quats)[n];
        sc_raw[0] = a.scales[3 * n]; sc_raw[1] = a.scales[3 * n + 1]; sc_raw[2] = a.scales[3 * n + 2];
        op_raw = a.opacities[n];
    }
    ShPrefetch pf;
    if (STAGE == 0 && DEG == 3 && prefetch_sh)
        sh_rows_issue(a.colors_in, a.sh_rest, n0, (int)min((int64_t)kProjThreads, a.N - n0), pf);

    bool vis = false;
    if (STAGE != 2) {
        Splat2D s;
        s.radius = 0; s.mx = s.my = s.depth = s.A = s.B = s.C = s.cxx = s.cyy = 0.f; s.x0 = s.x1 = s.y0 = s.y1 = 0;
        if (in_range) {
            const float quat[4] = {q4.x, q4.y, q4.z, q4.w};
            const float scale[3] = {act_scale(sc_raw[0], a.activations), act_scale(sc_raw[1], a.activations),
                                    act_scale(sc_raw[2], a.activations)};
            s = project_gaussian_cm<CAM, AA>(mean, quat, scale, cam, a.W, a.H, a.eps2d, a.near_p, a.far_p, a.radius_clip, GS_TILE, a.tw, a.th);
        }
        vis = s.radius > 0;
        if (!vis && in_range && a.rect_ref) a.rect_ref[f] = make_uint2(0u, 0u);
        int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        float op = 0.f, ex = -1.f, ey = -1.f;
        if (vis) {
            x0 = s.x0; x1 = s.x1; y0 = s.y0; y1 = s.y1;   // from the unrounded centre (gs_math.h: preal)
            if (a.rect_ref) a.rect_ref[f] = make_uint2(fp_span(x0, x1), fp_span(y0, y1));
            op = act_opacity(op_raw, a.activations);
            // antialiased mode: everything behind the projection sees op_eff = opacity * rho -- the record, the extents and the tile mask
            // below.  rho = 0 (a rank-deficient covariance) is an opacity of 0: no extent (alpha_extent's v > 1 test), an empty tight
            // rectangle, and in the full rectangle a record no pixel takes.
            if (AA) op *= s.rho;
            alpha_extent(op, s.cxx, s.cyy, ex, ey);
            // tight mode: keep only the tiles of the 3-sigma rectangle that hold a pixel centre where
            // alpha can reach 1/255 (the blend skips every other pixel anyway: identical image)
            if (a.tight) tile_rect_tight(s.mx, s.my, ex, ey, a.W, a.H, GS_TILE, x0, x1, y0, y1);
        }
        // tile footprint (gs_common.h: the footprint record): rectangle + (up to kMaskTiles tiles) a row-major bit per tile
        const int rw = x1 - x0, rect_tiles = rw * (y1 - y0);
        uint32_t tmask = fp_full_mask(rect_tiles);
        if (a.tight && rect_tiles > 0 && rect_tiles <= kMaskTiles) {
            // exact test per tile: some pixel centre of the tile must allow alpha >= 1/255
            const float tau = __log2f(255.f * op) + 0.02f, lim = tau + 1e-4f * fabsf(tau);
            const float qa = 0.5f * kLog2e * s.A, qb = kLog2e * s.B, qc = 0.5f * kLog2e * s.C;
            tmask = 0u;
            const float inv_rw = 1.0f / (float)rw;
            for (int i = 0; i < rect_tiles; ++i) {
                const int row = div_by_width(i, inv_rw), ty = y0 + row, tx = x0 + (i - row * rw);
                const float dx0 = (float)(tx * GS_TILE) + 0.5f - s.mx, dy0 = (float)(ty * GS_TILE) + 0.5f - s.my;
                if (quad_min_on_rect(qa, qb, qc, dx0, dx0 + (float)(GS_TILE - 1), dy0, dy0 + (float)(GS_TILE - 1)) <= lim) tmask |= 1u << i;
            }
        }
        const int cnt = rect_tiles <= kMaskTiles ? __popc(tmask) : rect_tiles;
        if (in_range) {
            a.radii[f] = s.radius;
            reinterpret_cast<float2*>(a.means2d)[f] = make_float2(s.mx, s.my);
            a.depths[f] = s.depth;
            a.conics[3 * f] = s.A; a.conics[3 * f + 1] = s.B; a.conics[3 * f + 2] = s.C;
            a.bbox[f] = fp_pack(x0, x1, y0, y1, tmask, (uint32_t)cnt);
            a.tiles_per_gauss[f] = cnt;
            if (AA) a.compensations[f] = vis ? s.rho : 0.f;
            if (vis) {
                // blend record: conic pre-scaled so the kernels evaluate exp2(-(hA dx^2 + B dx dy + hC dy^2))
                float4* r = a.rec + 3 * f;
                r[0] = make_float4(s.mx, s.my, 0.5f * kLog2e * s.A, kLog2e * s.B);
                r[1] = make_float4(0.5f * kLog2e * s.C, op, ex, ey);
            }
        }
    } else {
        vis = in_range && a.radii[f] > 0;
    }
    if (STAGE == 1) return;

    float rgb[3] = {0.5f, 0.5f, 0.5f};
    if (DEG >= 0) {
        vis_s[threadIdx.x] = vis ? 1 : 0;
        const int any_vis = __syncthreads_or(vis ? 1 : 0);
        if (any_vis) {
            const int rows = (int)min((int64_t)kProjThreads, a.N - n0);
            constexpr int ka3 = 3 * (DEG + 1) * (DEG + 1);
            if (STAGE == 0 && DEG == 3 && prefetch_sh) {
                sh_rows_commit(pf, a.sh_rest, n0, rows, tile);
            } else if (a.sh_rest) {
                if (DEG == 4) stage_sh_rows_split<25>(a.colors_in, a.sh_rest, n0, rows, 25, ka3, vis_s, tile);   // (SH4: K = 25)
                else if (a.K == 16) stage_sh_rows_split<16>(a.colors_in, a.sh_rest, n0, rows, 16, ka3, vis_s, tile);
                else stage_sh_rows_split<0>(a.colors_in, a.sh_rest, n0, rows, a.K, ka3, vis_s, tile);
            } else {
                if (DEG == 4) stage_sh_rows<25>(a.colors_in, n0, rows, 25, ka3, vis_s, tile);
                else if (a.K == 16) stage_sh_rows<16>(a.colors_in, n0, rows, 16, ka3, vis_s, tile);
                else stage_sh_rows<0>(a.colors_in, n0, rows, a.K, ka3, vis_s, tile);
            }
            __syncthreads();
            if (vis) {
                float ux, uy, uz;
                view_dir(mean, cam, ux, uy, uz);
                sh_to_rgb(DEG < 0 ? 0 : DEG, tile + threadIdx.x * (3 * a.K + 1), ux, uy, uz, rgb);
                if (DEG >= 1 && a.sh_jac) {
                    float G[12];
                    sh_dir_jacobian(DEG, tile + threadIdx.x * (3 * a.K + 1), ux, uy, uz, G);
                    // nine floats per Gaussian: eight as two aligned quads [C*N][8], the ninth in a plane of its own behind them
                    float4* jp = a.sh_jac + 2 * f;
                    jp[0] = make_float4(G[0], G[1], G[2], G[4]); jp[1] = make_float4(G[5], G[6], G[8], G[9]);
                    reinterpret_cast<float*>(a.sh_jac + 2 * (int64_t)a.C * a.N)[f] = G[10];
                }
            }
        }
    } else if (in_range) {
        const float* src = a.colors_in + 3 * (a.colors_per_camera ? f : n);
        rgb[0] = src[0]; rgb[1] = src[1]; rgb[2] = src[2];
    }
    if (in_range) {
        a.colors_out[3 * f] = rgb[0]; a.colors_out[3 * f + 1] = rgb[1]; a.colors_out[3 * f + 2] = rgb[2];
        if (vis) a.rec[3 * f + 2] = make_float4(rgb[0], rgb[1], rgb[2], 0.f);
    }
