// The body of one strip layer on the workgroup's frame, from the weight prologue to the last row's epilogue (see
// dense_strip_impl.h, which includes this file twice INSIDE a function template <int W, int KS> with `DenseStripArgs a` in scope:
// once as the whole body of the per-layer kernel and once as the device function the chained kernel calls per layer).  Text
// inclusion instead of a call from the kernel: an inlined call gives hipcc a different instruction order to allocate registers
// for, and the per-layer kernels - two of them at 256 VGPRs with nothing to spare - are to keep the listings they have.
// TN_STRIP_TID: the expression for the thread index (threadIdx.x in the kernel).  TN_STRIP_GEOM: the geometry type, DSGeom<W, KS> or
// (dense_strip_pair_w28.hip) DSGeomPair<KS>: two 28 x 28 frames per workgroup, 14 rows per wave.  No include guard on purpose.
  using G = TN_STRIP_GEOM;
  constexpr int H = W, NSU = G::NSU, K = KS * 32, KQ = G::KQ, ROWS = G::ROWS;
  constexpr bool ODD = (KS & 1) != 0;
  constexpr int XN = kXN, NPL = pl_len<KS>(), PLB = NPL < kPLB ? NPL : kPLB;
  static_assert(a_sched_complete<KS>(), "1x1 slot schedule leaves work unassigned");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = TN_STRIP_TID;
  if (a.ts && tid == 0) {
    a.ts[(size_t)blockIdx.x * 128 + 127] = __builtin_amdgcn_s_memtime();
    a.ts[(size_t)blockIdx.x * 128 + 126] = __builtin_amdgcn_s_memrealtime();     // 100 MHz
  }

  // ---- prologue: the layer's weights and tables -> LDS (once per launch) ----
  // LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction, no registers): every piece of the 72 + 4 (KQ + 1) KiB is in
  // flight at once and ONE wait follows.  Through registers (load, ds_write, 4 - 6 pieces per round trip) the copy took
  // 9 800 cycles at K = 320 - 13 % of a 28x28 launch, whose waves only have eight rows each to amortise it over.
  {
    typedef __attribute__((address_space(3))) void *lptr_t;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lptr_t)smem);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63;
    constexpr int P3 = kW3Bytes / 1024, P1 = (KQ + 1) * 4;
    const unsigned char *g3 = (const unsigned char *)a.w3s + ln * 16, *g1 = (const unsigned char *)a.w1s + ln * 16;
    for (int p = wv; p < P3; p += 4) dma16(g3 + p * 1024, lds0 + p * 1024);
    for (int p = wv; p < P1; p += 4) dma16(g1 + p * 1024, lds0 + G::W1OFF + p * 1024);
    f16 *t1 = (f16 *)(smem + G::T1OFF);      // (the constants ARE fp16 numbers: bn_relu_fold_fp16)
    for (int i = tid; i < K; i += 256) {
      t1[i] = (f16)a.s1[i];
      t1[K + i] = (f16)a.t1[i];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();

  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 31, h = lane >> 5;
  const int item = (int)(blockIdx.x % G::WGS) * 4 + wid;
  // (two frames per workgroup: waves 0 / 1 take the halves of the first frame, 2 / 3 of the second; wid is wave-uniform, and so
  // is the frame pointer below)
  const int pair = item % G::NPAIR, part = G::FPW == 2 ? (wid & 1) : item / G::NPAIR;
  const int r_lo = part * ROWS, r_hi = r_lo + ROWS;
  const int x = 14 * (2 * pair + (n >> 4)) - 1 + (n & 15);
  const bool xvalid = x >= 0 && x < W;
  const int xc = x < 0 ? 0 : (x >= W ? W - 1 : x);
  const int ldc = a.ldc;
  const unsigned rowpitch = (unsigned)W * ldc * 2;
  unsigned char *fb = (unsigned char *)(a.buf + (size_t)(G::FPW == 2 ? 2 * blockIdx.x + (wid >> 1) : blockIdx.x / G::WGS) * H * W * ldc);
  const unsigned colb = (unsigned)xc * ldc * 2 + 64 * h;     // full super-steps: 64 B per lane
  const unsigned colh = (unsigned)xc * ldc * 2 + 32 * h;     // the trailing half super-step: 32 B per lane
  const bool store_ok = (n & 15) >= 1 && (n & 15) <= 14 && xvalid;
  const unsigned outb = (unsigned)xc * ldc * 2 + K * 2 + 32 * h;
  const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(fb, 0, (int)((unsigned)H * rowpitch), 0x00020000);

  const unsigned char *w1l = smem + G::W1OFF + lane * 16;
  const unsigned char *w3l = smem + lane * 16;
  const f16 *tab1 = (const f16 *)(smem + G::T1OFF);
  // The paired geometry reads its weight fragments through three opaque base registers, 64 KiB apart (a ds_read's offset field
  // holds 16 bits).  From w1l / w3l hipcc forms a base register of its own per fragment past 64 KiB and keeps them all live across
  // the row loop: with the extra row event behind a 14-row loop (NREM = 1) that is five / six VGPRs too many at K = 288 / 320,
  // which went to scratch.  Same reads in the same slots; the one-frame instantiations keep the addresses they have.
  typedef __attribute__((address_space(3))) const unsigned char *lcp_t;
  unsigned lb0 = (unsigned)(size_t)(lcp_t)smem + lane * 16, lb1 = lb0 + 65536, lb2 = lb0 + 131072;
  if constexpr (G::FPW == 2) asm volatile("" : "+v"(lb0), "+v"(lb1), "+v"(lb2));
  auto lds_frag = [&](auto off_tag) TN_INL {      // the lane's 16 bytes of the 1 KiB fragment at byte OFF of the LDS image
    constexpr int OFF = decltype(off_tag)::value;
    const lcp_t b = (lcp_t)(size_t)(OFF < 65536 ? lb0 : OFF < 131072 ? lb1 : lb2);     // (pointer arithmetic: the offset folds into the read)
    return *(const __attribute__((address_space(3))) u32x4 *)(b + (OFF & 65535));
  };
  // the pixel fragment of the shift k-step: (1, 1, mask, 0, 0, 0, 0, 0) in the lanes that hold k = 0 .. 7
  const u32x4 xb_shift = {h == 0 ? 0x3c003c00u : 0u, (h == 0 && !xvalid) ? 0x0000fb53u : 0u, 0u, 0u};   // fp16 1.0 = 0x3c00, -60000 = 0xfb53

  // ================= state that lives across slots =================
  // every LDS read is issued at least two k-steps (6 - 8 slots, >= 200 cycles) ahead of its consumer: with one wave per SIMD
  // nothing else covers an exposed LDS round trip
  u32x4 ring[5][4];      // activation ring [super-step][k-step]: 16 B per lane = 8 channels of the lane's pixel; holds one row
  f32x16 acc[4];         // 1x1 accumulators [32-channel block]
  u32x4 wa[2][4];        // 1x1 weight fragments [k-step parity][block] (a register is reloaded for k-step + 2 behind its MFMA)
  u32x4 xb[XN];          // BN1 + ReLU'd pixel fragments [k-step % XN]: the BN pipeline runs up to XN - 2 k-steps ahead
  u32x4 cs[3], ct[3];    // BN1 constants [k-step % 3]: a / b of the lane's eight channels, packed halves
  u32x4 w3f[2][3];       // 3x3 weight fragments [step parity][dx] (reloaded for step + 2 behind their MFMA)
  f32x16 bacc[3];        // 3x3 accumulators [dx]
  unsigned e_pk[4];
  float o_c[2], o_l[2], o_r[2];
  unsigned o_pk[8];

  auto rowbase = [&](int y) TN_INL {
    const int yc = y < 0 ? 0 : (y >= H ? H - 1 : y);
    return fb + (unsigned)yc * rowpitch;
  };
  // ---------------- the BN pipeline: an ordered list of items per bottleneck row ----------------
  //   C(q)    the two ds_read_b128 of k-step q's BN1 constants
  //   BN(q).j BN1 + ReLU of dword j of k-step q's pixel fragment (2 VALU instructions: v_pk_fma_f16, v_pk_max_f16)
  //   LD(u).i one 16-byte activation load of the NEXT row into ring slot u, behind the last BN item that read the slot
  // in the order C0 C1 C2 | BN(0).0-3 C3 | BN(1).0-3 C4 | ... ; the list is consumed one item per slot, first by the spare slots
  // of the previous row's 3x3 phase (PLB items), then by the row's own 1x1 slots (see make_a_sched)
  auto ld_item = [&](auto u_tag, auto i_tag, int y) TN_INL {
    constexpr int U = decltype(u_tag)::value, I = decltype(i_tag)::value;
    constexpr bool HALF = ODD && U == NSU - 1;
    if ((TN_DS_EXP & 1) && y > r_lo + 1) return;
    if constexpr (HALF) ring[U][I] = *(const u32x4 *)(rowbase(y) + colh + 128 * U + 16 * I);
    else ring[U][I] = *(const u32x4 *)(rowbase(y) + colb + 128 * U + 16 * I);
  };
  auto consts_item = [&](auto q_tag) TN_INL {
    constexpr int Q = decltype(q_tag)::value;
    constexpr int U = Q >> 2, I = Q & 3;
    constexpr bool HALF = ODD && U == NSU - 1;
    const int c0 = (HALF ? 64 * U + 16 * h : 64 * U + 32 * h) + 8 * I;
    cs[Q % 3] = *(const u32x4 *)(tab1 + c0);
    ct[Q % 3] = *(const u32x4 *)(tab1 + K + c0);
  };
  auto bn_item = [&](auto q_tag, auto j_tag) TN_INL {
    constexpr int Q = decltype(q_tag)::value, J = decltype(j_tag)::value;
    const unsigned in = ring[Q >> 2][Q & 3][J];
    const unsigned sc = cs[Q % 3][J], sh = ct[Q % 3][J];
    unsigned o;      // clamp(x, lo, hi): BN1 + ReLU without arithmetic or rounding (calib_host.hip::bn_relu_clamp_fold; one statement: between two, hipcc pads the dependency with an s_nop)
    asm("v_pk_max_f16 %0, %1, %2\n\tv_pk_min_f16 %0, %0, %3" : "=&v"(o) : "v"(in), "v"(sc), "v"(sh));
    xb[Q % XN][J] = o;
  };
  // pipeline item IDX of the row ybn
  auto pl_item = [&](auto idx_tag, int ybn) TN_INL {
    constexpr PItem it = pl_at<KS>(decltype(idx_tag)::value);
    if constexpr (it.kind == 1) consts_item(ic<it.q>{});
    else if constexpr (it.kind == 2) bn_item(ic<it.q>{}, ic<it.j>{});
    else if constexpr (it.kind == 3) ld_item(ic<it.q>{}, ic<it.j>{}, ybn + 1);
  };
  auto wa_item = [&](auto q_tag, auto mb_tag) TN_INL {
    constexpr int Q = decltype(q_tag)::value, MB = decltype(mb_tag)::value;
    if ((TN_DS_EXP & 16) && Q >= 2) return;     // (timing experiment: the 1x1 phase keeps reusing its first eight weight fragments)
    if constexpr (G::FPW == 2) wa[Q & 1][MB] = lds_frag(ic<G::W1OFF + (Q * 4 + MB) * 1024>{});
    else wa[Q & 1][MB] = *(const u32x4 *)(w1l + (Q * 4 + MB) * 1024);
  };
  auto wa_group = [&](auto q_tag) TN_INL { static_for<4>([&](auto mb_tag) TN_INL { wa_item(q_tag, mb_tag); }); };
  // what the 3x3 phase of the previous row would have done for this row (first rows of a wave)
  auto prologue_exposed = [&](int ybn) TN_INL {
    wa_group(ic<0>{});
    wa_group(ic<1>{});
    static_for<PLB>([&](auto i_tag) TN_INL { pl_item(i_tag, ybn); });
    TN_SB();
  };

  // ---- epilogue A: acc (= BN2 applied) -> ReLU, one rounding to fp16, lane-local pack -> window row PROW; 40 items: per window
  // tuple T (k-step of the 3x3: accumulators 8 (T & 1) .. + 7 of block T >> 1) four convert + ReLU items of two values each and
  // the window write ----
  auto epa_item = [&](auto prow_tag, auto e_tag) TN_INL {
    constexpr int PROW = decltype(prow_tag)::value, E = decltype(e_tag)::value;
    constexpr int T = E / 5, I = E % 5, MB = T >> 1, R0 = 8 * (T & 1);
    unsigned (&epk)[4] = e_pk;             // (asm operands alone do not capture in a generic lambda)
    f32x16 (&accr)[4] = acc;
    if constexpr (I < 4) {
      const float a0 = accr[MB][R0 + 2 * I], a1 = accr[MB][R0 + 2 * I + 1];
      asm("v_cvt_pk_f16_f32 %0, %1, %2\n\tv_pk_max_f16 %0, %0, 0" : "=v"(epk[I]) : "v"(a0), "v"(a1));
    } else {
      win_write<PROW, T>(epk[0], epk[1], epk[2], epk[3]);
    }
  };
  auto epilogue_a_exposed = [&](auto prow_tag) TN_INL {
    static_for<40>([&](auto e_tag) TN_INL { epa_item(prow_tag, e_tag); });
    TN_SB();
  };
  // ---- epilogue B: 24 items; output dword P = out channels 16 h + 2 P, + 1 of the lane's pixel: out[x] = acc[dx=0][x] +
  // acc[dx=-1][x-1] + acc[dx=+1][x+1], fp16; 16 B stored behind every fourth dword.  `off`: byte offset of the lane's 32 B (halo
  // lanes / no previous row: past the descriptor's range - the hardware drops the store, no branch) ----
  auto epb_item = [&](auto i_tag, unsigned off) TN_INL {
    constexpr int I = decltype(i_tag)::value, P = I / 3, PART = I % 3;
    if constexpr (PART == 0) {
      o_c[0] = bacc[1][2 * P]; o_c[1] = bacc[1][2 * P + 1];
      o_l[0] = bacc[0][2 * P]; o_l[1] = bacc[0][2 * P + 1];
    } else if constexpr (PART == 1) {
      o_c[0] += dpp_f32<0x111>(o_l[0]);     // row_shr:1: lane x reads lane x - 1
      o_c[1] += dpp_f32<0x111>(o_l[1]);
      o_r[0] = bacc[2][2 * P]; o_r[1] = bacc[2][2 * P + 1];
    } else {
      o_c[0] += dpp_f32<0x101>(o_r[0]);     // row_shl:1: lane x reads lane x + 1
      o_c[1] += dpp_f32<0x101>(o_r[1]);
      const h2_t p = {(f16)o_c[0], (f16)o_c[1]};
      o_pk[P] = __builtin_bit_cast(unsigned, p);
      if constexpr (P == 3 || P == 7) {
        const u32x4 o = {o_pk[P - 3], o_pk[P - 2], o_pk[P - 1], o_pk[P]};
        __builtin_amdgcn_raw_buffer_store_b128(o, orsrc, off + (P == 7 ? 16 : 0), 0, 0);
      }
    }
  };
  auto out_offset = [&](int yo, bool valid) TN_INL { return (valid && store_ok) ? outb + (unsigned)yo * rowpitch : 0x80000000u; };
  // (belt and braces: the 3x3 phase's last statement already carries these wait states, mfma32_win_last3)
  auto bacc_ready = [&]() TN_INL {   // an asm MFMA's result may be read by anything but the next MFMA of its chain only 18+ wait states after issue
    f32x16 (&b)[3] = bacc;
    asm volatile("s_nop 15\n\ts_nop 3" : "+a"(b[0]), "+a"(b[1]), "+a"(b[2]));
  };
  auto epilogue_b_exposed = [&](int yo) TN_INL {
    bacc_ready();
    const unsigned off = out_offset(yo, true);
    static_for<24>([&](auto i_tag) TN_INL { epb_item(i_tag, off); TN_SB(); });
  };
  auto w3_item = [&](auto s_tag, auto dx_tag) TN_INL {
    constexpr int S = decltype(s_tag)::value, DX = decltype(dx_tag)::value;
    if ((TN_DS_EXP & 8) && S >= 2) return;      // (timing experiment: the 3x3 phase keeps reusing its first six weight fragments)
    if constexpr (G::FPW == 2) w3f[S & 1][DX] = lds_frag(ic<(S * 3 + DX) * 1024>{});
    else w3f[S & 1][DX] = *(const u32x4 *)(w3l + (S * 3 + DX) * 1024);
  };

  // ================= 1x1 phase of bottleneck row yb (its first PLB pipeline items have run) =================
  // a slot: the MFMA, the reload of its weight register for k-step + 2, and ONE item: the next of the row's BN pipeline (when the
  // pipeline would otherwise fall behind the MFMAs) or the next of the previous output row's epilogue B (make_a_sched)
  auto phase_a = [&](int yb, int yo_prev, bool prev_valid) TN_INL {
    constexpr auto SA = make_a_sched<KS>();
    bacc_ready();
    const unsigned off_prev = out_offset(yo_prev, prev_valid);
    static_for<KQ + 1>([&](auto q_tag) TN_INL {
      constexpr int Q = decltype(q_tag)::value;
      static_for<4>([&](auto mb_tag) TN_INL {
        constexpr int MB = decltype(mb_tag)::value, SL = 4 * Q + MB;
        if constexpr (MB == 0) {     // one wait for the four weight fragments of the k-step (requested two k-steps ago); inputs only:
          u32x4 (&w)[4] = wa[Q & 1];   // an output would draw hipcc's asm boundary pad (s_nop) in front of the MFMA
          asm volatile("" :: "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]));
        }
        if constexpr (Q == 0) {
          f32x16 z;
#pragma unroll
          for (int i = 0; i < 16; ++i) z[i] = 0.f;
          acc[MB] = mfma32(wa[0][MB], xb[0], z);
        } else if constexpr (Q == KQ) {
          acc[MB] = mfma32(wa[Q & 1][MB], xb_shift, acc[MB]);
        } else {
          acc[MB] = mfma32(wa[Q & 1][MB], xb[Q % XN], acc[MB]);
        }
        if constexpr (Q + 2 < KQ + 1) wa_item(ic<Q + 2>{}, mb_tag);
        constexpr ASlot sl = SA.s[SL];
        static_for<sl.npl>([&](auto k_tag) TN_INL { pl_item(ic<sl.pl0 + decltype(k_tag)::value>{}, yb); });
        static_for<sl.nepb>([&](auto k_tag) TN_INL { epb_item(ic<sl.epb0 + decltype(k_tag)::value>{}, off_prev); });
        TN_WIN_FENCE();
        TN_SB();
      });
    });
  };

  // ================= 3x3 phase of one output row: window rows (ROT + 1) % 3, (ROT + 2) % 3, ROT (the new one) =================
  // slot (dy, k-step, dx): the MFMA, the reload of its weight register for step + 2, and one item: slots 0 - 39 epilogue A of the
  // new row into window row ROT (first needed by slot 48), 40 / 41 the next row's first weight fragments, 42 - 71 the first PLB
  // items of the next row's BN pipeline
  auto phase_b = [&](auto rot_tag, auto epa_tag, int ybn) TN_INL {
    constexpr int ROT = decltype(rot_tag)::value;
    constexpr bool HAS_EPA = decltype(epa_tag)::value != 0;
    static_for<72>([&](auto e_tag) TN_INL {
      constexpr int E = decltype(e_tag)::value;
      constexpr int S = E / 3, DX = E % 3, DY = S / 8, T = S % 8;
      constexpr int PROW = (ROT + 1 + DY) % 3;
      if constexpr (DX == 0) {     // one wait for the step's three weight fragments
        u32x4 (&w)[3] = w3f[S & 1];
        asm volatile("" :: "v"(w[0]), "v"(w[1]), "v"(w[2]));
      }
      if constexpr (S < 23) mfma32_win<S == 0, PROW, T>(bacc[DX], w3f[S & 1][DX]);
      else if constexpr (DX == 2) mfma32_win_last3<PROW, T>(bacc[0], bacc[1], bacc[2], w3f[S & 1][0], w3f[S & 1][1], w3f[S & 1][2]);
      if constexpr (S + 2 < 24) w3_item(ic<S + 2>{}, ic<DX>{});
      if constexpr (E < 40) {
        if constexpr (HAS_EPA) epa_item(rot_tag, e_tag);
      } else if constexpr (E < 42) {
        wa_group(ic<E - 40>{});
      } else if constexpr (E - 42 < PLB) {
        pl_item(ic<E - 42>{}, ybn);
      }
      TN_WIN_FENCE();
      TN_SB();
    });
  };
  auto load_w3_first = [&]() TN_INL { static_for<6>([&](auto i_tag) TN_INL { w3_item(ic<decltype(i_tag)::value / 3>{}, ic<decltype(i_tag)::value % 3>{}); }); };

  int nstamp = 0;
  auto stamp = [&]() TN_INL {
    if (a.ts && wid == 0 && nstamp < 125) {
      if (lane == 0) a.ts[(size_t)blockIdx.x * 128 + nstamp] = __builtin_amdgcn_s_memtime();
      ++nstamp;
    }
  };
  // one steady-state row: bottleneck row yb (1x1 phase, into window row ROT through the 3x3 phase's fillers), output row yb - 1
  auto row_event = [&](auto rot_tag, int yb, bool prev_valid) TN_INL {
    stamp();
    if (!(TN_DS_EXP & 4)) phase_a(yb, yb - 2, prev_valid);
    load_w3_first();
    TN_SB();
    stamp();
    if (!(TN_DS_EXP & 2)) phase_b(rot_tag, ic<1>{}, yb + 1);
  };

  // ================= the wave's program =================
  {   // accumulators of the 3x3 start defined (the first 1x1 phases run an epilogue B whose store is dropped)
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    bacc[0] = z; bacc[1] = z; bacc[2] = z;
  }
  stamp();
  const int yfirst = r_lo > 0 ? r_lo - 1 : 0;
  static_for<NSU>([&](auto u_tag) TN_INL {
    constexpr bool HALF = ODD && decltype(u_tag)::value == NSU - 1;
    static_for<(HALF ? 2 : 4)>([&](auto i_tag) TN_INL { ring[decltype(u_tag)::value][decltype(i_tag)::value] =
        *(const u32x4 *)(rowbase(yfirst) + (HALF ? colh : colb) + 128 * decltype(u_tag)::value + 16 * decltype(i_tag)::value); });
  });
  // bottleneck row r_lo - 1 -> window row 0 (zeros above the image)
  if (r_lo > 0) {
    prologue_exposed(r_lo - 1);
    phase_a(r_lo - 1, 0, false);
    epilogue_a_exposed(ic<0>{});
  } else {
    win_zero<0>();
  }
  // bottleneck row r_lo -> window row 1
  prologue_exposed(r_lo);
  phase_a(r_lo, 0, false);
  epilogue_a_exposed(ic<1>{});
  prologue_exposed(r_lo + 1);
  stamp();
  // rows r_lo + 1 .. r_hi - 1: the steady state, window rotation 2, 0, 1, ...
  int yb = r_lo + 1;
  for (; yb + 2 < r_hi; yb += 3) {
    row_event(ic<2>{}, yb, yb > r_lo + 1);
    row_event(ic<0>{}, yb + 1, true);
    row_event(ic<1>{}, yb + 2, true);
  }
  constexpr int NREM = (ROWS - 1) % 3;          // steady-state rows left over
  if constexpr (NREM >= 1) { row_event(ic<2>{}, yb, yb > r_lo + 1); ++yb; }
  if constexpr (NREM >= 2) { row_event(ic<0>{}, yb, true); ++yb; }
  // bottleneck row r_hi (zeros below the image) -> window row (ROWS + 1) % 3, output row r_hi - 1
  constexpr int ROTL = (ROWS + 1) % 3;
  if (r_hi < H) {
    row_event(ic<ROTL>{}, r_hi, true);
  } else {
    epilogue_b_exposed(r_hi - 2);
    win_zero<ROTL>();
    load_w3_first();
    TN_SB();
    phase_b(ic<ROTL>{}, ic<0>{}, r_hi);
  }
  stamp();
  epilogue_b_exposed(r_hi - 1);
  stamp();
  if (a.ts && wid == 0 && lane == 0) a.ts[(size_t)blockIdx.x * 128 + 125] = __builtin_amdgcn_s_memrealtime();
