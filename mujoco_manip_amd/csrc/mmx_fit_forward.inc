// The forward pass, the activation saving and the backward delta pass of one optimisation step, stated once for both
// objectives: mmx_policy_fit.hip includes this file twice, with FIT_PG 0 (mmx_fit_forward_kernel: the mean-squared
// error) and FIT_PG 1 (mmx_pg_forward_kernel: PPO's clipped surrogate; G: its arrays and scalars, mmx_pg.h).  The two
// differ in the output delta and in what a tile sums: the squared errors, or the three statistics.  (An include and
// not a template: the kernels take their arguments by value, and the first one's instructions stay what they were.)
extern "C" __global__ void __launch_bounds__(kThreads)
#if FIT_PG
mmx_pg_forward_kernel(MmxPolicy P, MmxFit F, MmxPg G) {
#else
mmx_fit_forward_kernel(MmxPolicy P, MmxFit F) {
#endif
  __shared__ __attribute__((aligned(16))) float buf[2][POLICY_MAX_WIDTH * kTS];  // [unit][sample], ping-pong
  __shared__ int64_t pair[kTS];
  __shared__ float sq[kTS * POLICY_MAX_ADIM];   // MSE: the errors; PG: z' [sample][component]
#if FIT_PG
  __shared__ float zsh[kTS * POLICY_MAX_ADIM];  // z [sample][component]
  float zn[kTS], sigma = 0.f;  // thread a < A: its component's z' per sample, and sigma_a
#endif
  const int tid = threadIdx.x, B = F.B;
  const int s0 = (int)blockIdx.x * kTS;
  const int ns = min(kTS, B - s0);  // the tile's real samples; the others compute on pair 0's data and store nothing
  const float* data = policy_data(P);
  const int L = policy_u(P.n_layers), activation = policy_u(P.activation), A = policy_u(P.A);

  if (tid < kTS)
    pair[tid] = tid < ns ? policy_fit_index(F.shuffle, F.seed_lo, F.seed_hi, F.k, (uint32_t)(s0 + tid), (uint32_t)B, F.n) : 0;
  __syncthreads();
  float* x0 = F.ws;  // x_0 [B][85]
  for (int e = tid; e < kTS * POLICY_NOBS; e += kThreads) {
    const int s = e / POLICY_NOBS, c = e - s * POLICY_NOBS;
    const float v = policy_normalise(F.obs[(size_t)pair[s] * POLICY_NOBS + (size_t)c], data[P.shift_off + c], data[P.scale_off + c]);
    buf[0][c * kTS + s] = v;
    if (s < ns) x0[(size_t)(s0 + s) * POLICY_NOBS + (size_t)c] = v;
  }
  __syncthreads();

  // ---- forward: src -> dst, thread j = neuron j of the layer (its padding neurons, weights 0, give act(0) = 0)
  size_t xoff = 0, doff = F.d_base;  // x_l and d_l in the workspace, kept current layer by layer
  int cur = 0;
  for (int l = 0; l < L; l++) {
    const int in = policy_u(P.in[l]), out = policy_u(P.out[l]), outp = policy_padded(out);
    const bool last = l + 1 == L;
    xoff += (size_t)in * (size_t)B;  // x_{l+1}
    const float* src = buf[cur];
    float* dst = buf[cur ^ 1];
    if (tid < outp) {
      policy_gptr w = (policy_gptr)(data + policy_u(P.woff[l])) + tid;
      float acc[kTS];
      const float bias = data[policy_u(P.boff[l]) + tid];
#pragma unroll
      for (int s = 0; s < kTS; s++) acc[s] = bias;
#pragma unroll 2
      for (int k = 0; k < in; k++) {
        const float wk = w[(size_t)k * (size_t)outp];
        const f32x4* xs = (const f32x4*)(src + k * kTS);
#pragma unroll
        for (int q = 0; q < kTS / 4; q++) {
          const f32x4 xv = xs[q];
          acc[4 * q + 0] = fmaf(wk, xv.x, acc[4 * q + 0]);
          acc[4 * q + 1] = fmaf(wk, xv.y, acc[4 * q + 1]);
          acc[4 * q + 2] = fmaf(wk, xv.z, acc[4 * q + 2]);
          acc[4 * q + 3] = fmaf(wk, xv.w, acc[4 * q + 3]);
        }
      }
      if (!last) {
        float* xn = F.ws + xoff;  // x_{l+1} [B][out]
#pragma unroll
        for (int s = 0; s < kTS; s++) {
          const float a = policy_activate(activation, acc[s]);
          dst[tid * kTS + s] = a;
          if (s < ns && tid < out) xn[(size_t)(s0 + s) * (size_t)out + (size_t)tid] = a;
        }
      }
#if FIT_PG
      else {
        // z and z' of this thread's component into LDS: every sample's ratio needs all A of them
        if (tid < A) {
          sigma = data[policy_u(P.std_off) + tid];
#pragma unroll
          for (int s = 0; s < kTS; s++) {
            const size_t e = (size_t)pair[s] * (size_t)A + (size_t)tid;
            const float z = G.noise[e];
            zn[s] = pg_znew(sigma, z, G.mean_old[e], acc[s]);
            zsh[s * POLICY_MAX_ADIM + tid] = z;
            sq[s * POLICY_MAX_ADIM + tid] = zn[s];
          }
        }
      }
#else
      else if (tid < A) {
        // the output delta into dst, the squared errors for the tile's loss partial
        float* dl = F.ws + doff;
#pragma unroll
        for (int s = 0; s < kTS; s++) {
          const float y = F.target[(size_t)pair[s] * (size_t)A + (size_t)tid];
          const float e = acc[s] - y, dv = policy_fit_out_delta(acc[s], y, F.dscale);
          sq[s * POLICY_MAX_ADIM + tid] = e;
          dst[tid * kTS + s] = dv;
          if (s < ns) dl[(size_t)(s0 + s) * (size_t)A + (size_t)tid] = dv;
        }
      }
#endif
    }
#if FIT_PG
    {
      if (last) {  // (uniform: every thread of the workgroup takes this barrier, outside the tid < outp branch)
        __syncthreads();
        if (tid < A) {
          // each of the A threads forms every sample's ratio itself, from the same LDS values in the same order:
          // the same bits, and no second exchange.  Thread 0 also sums the tile's statistics, samples in order
          float* dl = F.ws + doff;
          float st0 = 0.f, st1 = 0.f, st2 = 0.f;
#pragma unroll
          for (int s = 0; s < kTS; s++) {
            float lr = 0.f;
            for (int a = 0; a < A; a++) lr = pg_log_ratio_add(lr, zsh[s * POLICY_MAX_ADIM + a], sq[s * POLICY_MAX_ADIM + a]);
            const PgSample q = pg_sample(lr, G.adv[pair[s]], G.invB, G.lo, G.hi);
            const float dv = pg_out_delta(q.g, zn[s], sigma);
            dst[tid * kTS + s] = dv;
            if (s < ns) {
              dl[(size_t)(s0 + s) * (size_t)A + (size_t)tid] = dv;
              st0 += q.loss, st1 += q.kl, st2 += q.clipped;
            }
          }
          if (tid == 0) {
            float* sp = F.ws + G.stat_base + (size_t)blockIdx.x * 3;
            sp[0] = st0, sp[1] = st1, sp[2] = st2;
          }
        }
      }
    }
#endif
    __syncthreads();
    cur ^= 1;
    if (!last) doff += (size_t)out * (size_t)B;
  }
#if !FIT_PG
  if (tid == 0) {
    float acc = 0.f;
    for (int s = 0; s < ns; s++)
      for (int a = 0; a < A; a++) acc = fmaf(sq[s * POLICY_MAX_ADIM + a], sq[s * POLICY_MAX_ADIM + a], acc);
    F.ws[F.loss_base + blockIdx.x] = acc;
  }
#endif

  // ---- backward: buf[cur] holds d_{l+1} [unit][sample]; thread c = unit c of layer l reads row c of W_{l+1}
  for (int l = L - 2; l >= 0; l--) {
    const int out = policy_u(P.out[l]), nout = policy_u(P.out[l + 1]), noutp = policy_padded(nout);
    const float* src = buf[cur];
    float* dst = buf[cur ^ 1];
    xoff -= (size_t)out * (size_t)B;   // x_{l+1} [B][out_l]
    doff -= (size_t)out * (size_t)B;   // d_l
    if (tid < out) {
      policy_gptr w = (policy_gptr)(data + policy_u(P.woff[l + 1])) + (size_t)tid * (size_t)noutp;
      float acc[kTS];
#pragma unroll
      for (int s = 0; s < kTS; s++) acc[s] = 0.f;
#pragma unroll 2
      for (int j = 0; j < nout; j++) {
        const float wj = w[j];
        const f32x4* ds = (const f32x4*)(src + j * kTS);
#pragma unroll
        for (int q = 0; q < kTS / 4; q++) {
          const f32x4 dv = ds[q];
          acc[4 * q + 0] = fmaf(wj, dv.x, acc[4 * q + 0]);
          acc[4 * q + 1] = fmaf(wj, dv.y, acc[4 * q + 1]);
          acc[4 * q + 2] = fmaf(wj, dv.z, acc[4 * q + 2]);
          acc[4 * q + 3] = fmaf(wj, dv.w, acc[4 * q + 3]);
        }
      }
      // the saved activation of this unit: x_{l+1}, written above by this very thread
      const float* xn = F.ws + xoff;
      float* dl = F.ws + doff;
#pragma unroll
      for (int s = 0; s < kTS; s++) {
        const float a = s < ns ? xn[(size_t)(s0 + s) * (size_t)out + (size_t)tid] : 0.f;
        const float dv = policy_fit_hidden_delta(activation, acc[s], a);
        dst[tid * kTS + s] = dv;
        if (s < ns) dl[(size_t)(s0 + s) * (size_t)out + (size_t)tid] = dv;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}
