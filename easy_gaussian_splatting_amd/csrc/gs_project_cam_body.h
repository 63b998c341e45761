// The body of project_cam_kernel / project_cam_cm_kernel (gs_project.hip), which define DEG, SUMS, the camera model CAM and the
// antialiased mode AA around it.
// Included once per kernel template, inside its braces: no include guard, nothing but the body.
    __shared__ float lds_cam[32];
    __shared__ double wave_sums[kProjThreads / 64][16];
    if (guard_tripped(a.guard)) return;
    const int c = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * kProjThreads + threadIdx.x;
    const int64_t f = (int64_t)c * a.N + n;
    Camera cam;
    load_camera(a.viewmats, a.Ks, c, a.W, a.H, lds_cam, cam);
    double acc[kCamTerms];
#pragma unroll
    for (int i = 0; i < kCamTerms; ++i) acc[i] = 0.0;
    if (n < a.N && a.radii[f] > 0) {
        const float mean[3] = {a.means[3 * n], a.means[3 * n + 1], a.means[3 * n + 2]};
        const float4 q4 = reinterpret_cast<const float4*>(a.quats)[n];
        const float quat[4] = {q4.x, q4.y, q4.z, q4.w};
        const float scale[3] = {act_scale(a.scales[3 * n], a.activations), act_scale(a.scales[3 * n + 1], a.activations),
                                act_scale(a.scales[3 * n + 2], a.activations)};
        if (DEG >= 1) {   // the SH colour's dependence on the camera centre: minus the direction term of v_mean
            const float rgb[3] = {a.colors_post[3 * f], a.colors_post[3 * f + 1], a.colors_post[3 * f + 2]};
            float v_rgb[3];
            if (SUMS) { const float4 z = a.row_sums[3 * f + 2]; v_rgb[0] = z.x; v_rgb[1] = z.y; v_rgb[2] = z.z; }
            else { v_rgb[0] = a.v_colors_post[3 * f]; v_rgb[1] = a.v_colors_post[3 * f + 1]; v_rgb[2] = a.v_colors_post[3 * f + 2]; }
            float ux, uy, uz, term[3];
            const float dn = view_dir(mean, cam, ux, uy, uz);
            if (a.sh_jac) {   // (project_bwd_kernel's layout)
                float G[12];
                const float4 j0 = a.sh_jac[2 * f], j1 = a.sh_jac[2 * f + 1];
                G[10] = reinterpret_cast<const float*>(a.sh_jac + 2 * (int64_t)gridDim.y * a.N)[f];
                G[0] = j0.x; G[1] = j0.y; G[2] = j0.z; G[4] = j0.w; G[5] = j1.x; G[6] = j1.y; G[8] = j1.z; G[9] = j1.w;
                sh_dir_term_jac(DEG, G, rgb, v_rgb, ux, uy, uz, dn, term);
            } else {
                sh_dir_term(DEG, a.sh_from_1 + a.sh_stride * n, rgb, v_rgb, ux, uy, uz, dn, term);
            }
            acc[12] = -(double)term[0]; acc[13] = -(double)term[1]; acc[14] = -(double)term[2];
        }
        ProjChainT<preal> p;
        if (project_chain<preal, CAM, AA>(mean, quat, scale, cam, a.eps2d, a.near_p, a.far_p, p)) {
            float v_mean[3] = {0.f, 0.f, 0.f}, v_quat[4] = {0.f, 0.f, 0.f, 0.f}, v_scale[3] = {0.f, 0.f, 0.f};   // (not used here)
            float2 vm;
            float vc[3];
            if (SUMS) {
                const float4 x = a.row_sums[3 * f], y = a.row_sums[3 * f + 1];
                vm = make_float2(x.x, x.y); vc[0] = y.x; vc[1] = y.y; vc[2] = y.z;
            } else {
                vm = reinterpret_cast<const float2*>(a.v_means2d)[f];
                vc[0] = a.v_conics[3 * f]; vc[1] = a.v_conics[3 * f + 1]; vc[2] = a.v_conics[3 * f + 2];
            }
            if (AA) {   // (project_bwd_kernel's v_rho, from the record-opacity gradient it left per (camera, Gaussian))
                const preal v_rho = (preal)a.v_op_rec[f] * (preal)act_opacity(a.opacities[n], a.activations);
                project_vjp_cam<preal, CAM, AA>(mean, scale, cam, p, vm.x, vm.y, vc[0], vc[1], vc[2], 0.f, v_mean, v_quat, v_scale, acc, acc + 9, v_rho, (preal)a.eps2d);
            } else
            project_vjp_cam<preal, CAM>(mean, scale, cam, p, vm.x, vm.y, vc[0], vc[1], vc[2], 0.f, v_mean, v_quat, v_scale, acc, acc + 9);
        }
    }
    const int lane = lane_id(), wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < kCamTerms; ++i) {
        const double t = wave_reduce_add(acc[i]);
        if (lane == 0) wave_sums[wave][i] = t;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        double t = 0.0;
        if (threadIdx.x < kCamTerms) {
#pragma unroll
            for (int w = 0; w < kProjThreads / 64; ++w) t += wave_sums[w][threadIdx.x];
        }
        a.cam_partials[((int64_t)c * gridDim.x + blockIdx.x) * 16 + threadIdx.x] = t;
    }
