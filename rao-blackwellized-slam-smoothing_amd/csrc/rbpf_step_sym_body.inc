// The step of one particle by one workgroup on block-lower storage: the statements of step_sym_kernel<TS, D, NS, WR, E, CH>, included
// as the body of that kernel and of step_sym_body (rbpf_step_sym.hip).  Expects the template parameters TS, D, NS, WR, E, CH and the
// arguments `a` (StepArgs) in scope.  Kept as text so that the kernel compiles to exactly what it did when the statements stood in it:
// through a call, even a forced-inline one, twenty instantiations came out with other register counts.
  const int chv = CH ? CH : a.lay.CH64;                        // tile rows (CH = 0: 6, 10, 12 or 14, from the layout)
  const int NW = sym_waves(chv), NT = 64 * NW;                 // CH = 16: eight waves, one workgroup per CU (the same eight waves per CU as 2 x 4)
  constexpr int NPH = sym_phases(CH);                          // column phases (waves per row pair; CH = 0: one)
  constexpr bool kGStrip = (CH == 16 || CH == 0);              // column strips in the global workspace, one block column staged in LDS
  extern __shared__ double smem[];
  constexpr int DE = D + E, ND = NS * D, NDA = ND > 0 ? ND : 1, NSA = NS > 0 ? NS : 1;
  // more than four pending sets in a flush: the wave's two tile rows go through every block column one after the other, so that
  // the row factors KS(r, .) of ONE row (NS * D registers) are live at a time
  constexpr bool kSplit = WR && NS > 4;
  const ModelDev& M = a.mdl;
  const Layout& Ly = a.lay;
  const int n = Ly.n, nb = Ly.nb, mc = Ly.mc, ldx = Ly.ldx, ldb = Ly.ldb;
  const int pos = xcd_position((int)blockIdx.x, (int)gridDim.x);   // processing position (sorted by the matrix the particle reads)
  const int* pre_i = a.pre_i + (size_t)pos * kPreInts;
  if (a.phase >= 0 && pre_i[5] != a.phase) return;      // single-bank flush: not this launch's share (workgroup-uniform)
  const int i = pre_i[0];
  const int dslot = WR ? pre_i[4] : i;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SymPlan lp = sym_plan(n, DE, ldx, M.ktot, WR ? ND : 0, chv, ((RBPF_SYM_LIGHT_WGS > 2 && !WR && E == 0) || kGStrip) ? 0 : 1);
  double* Hs = smem + lp.off_H + ((nb * DE) & 1);             // [H | ivec] of column c at Hs[c * DE ..): core pairs 16-byte aligned
  double* xls = smem + lp.off_xl;
  double* PHt = smem + lp.off_PHt;                            // [DE][ldx]
  double* tabS = smem + lp.off_tab;
  double* tabC = tabS + (M.ktot > 0 ? M.ktot : 1);
  double* misc = smem + lp.off_misc;
  double* red = smem + lp.off_red;
#ifdef RBPF_SYM_DIAG_SAMEBASE                    // timing experiment only (wrong results): every particle streams one of 64 matrices
  const int ancb = pre_i[2], baseb = pre_i[3] & 63;
#else
  const int ancb = pre_i[2], baseb = pre_i[3];
#endif
  // sharded filter: a bank index >= n_bank_local refers to a received record [T | B | F | xl] (same layout as the banks)
  const bool remote = a.rec != nullptr && ancb >= a.n_bank_local;
  const double* recp = remote ? a.rec + (size_t)(ancb - a.n_bank_local) * a.rec_stride : nullptr;
  const bool remoteP = a.rec != nullptr && baseb >= a.n_bank_local;
  const double* recP = remoteP ? a.rec + (size_t)(baseb - a.n_bank_local) * a.rec_stride : nullptr;
  const TS* srcT = remoteP ? reinterpret_cast<const TS*>(recP) : reinterpret_cast<const TS*>(a.Pt_old) + (size_t)baseb * a.Pt_old_stride;
  const TS* srcB = remoteP ? reinterpret_cast<const TS*>(recP + a.rec_off_B) : reinterpret_cast<const TS*>(a.Pb_old) + (size_t)baseb * a.Pb_old_stride;
  const double* srcX = remote ? recp + a.rec_off_X : a.xl_old + (size_t)ancb * a.xl_old_stride;
  const double* Fs[NSA];
#pragma unroll
  for (int s = 0; s < NSA; ++s) Fs[s] = nullptr;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (a.fset[s]) Fs[s] = a.fset[s] + (size_t)pre_i[kPreSet0 + s] * 2 * D * ldx;
    else Fs[s] = remote ? recp + a.rec_off_F : a.F_old + (size_t)ancb * 2 * D * ldx;
  }

  RBPF_SYM_KSTAMP(0);
  // ---- A: propagated state (propagate_kernel ran first), prior mean ----
  // The prologue pays one dependent global latency, that of pre_i above: whatever hangs on `pos` or on the thread alone is asked for
  // here, next to it.  Phase B reads the propagated position itself (a workgroup-uniform address), not through `misc` and a barrier
  // of its own; Rnb reaches phase C through `misc` as before, behind the barrier that the tables need anyway.  (All seventeen doubles
  // as scalars cost the read-only kernels eight spilled SGPRs, the VGPR that holds them, and with it 28 bytes of scratch in the stream.)
  const double* pre_d = a.pre_d + (size_t)pos * kPreDoubles;
  const double px0 = pre_d[0], px1 = pre_d[1], px2 = pre_d[2];
  // Jacobian columns: loop index ci = tid, tid + NT, ... forms column (ci + crot) mod n.  dense-mag rotates by three: the basis columns
  // (nine divisions each) fill whole rounds of the workgroup, and the identity columns c < 3, which cost nothing, are the remainder
  // (n = 515: two full rounds, then three lanes of copies -- not three lanes of divisions while every other wave waits).  These
  // columns feed no reduction here, so the mapping is free.  The basis indices of a thread's first kNNPre columns are asked for now.
  constexpr int kNNPre = 2;
  const int crot = (M.kind == 1) ? 3 : 0;
  auto jcol = [&](int ci) { const int c = ci + crot; return c >= n ? c - n : c; };
  int nnp[kNNPre][3] = {};
  if (a.H_ext == nullptr) {
#pragma unroll
    for (int it = 0; it < kNNPre; ++it)
      if (tid + it * NT < n) H_column_indices(M, jcol(tid + it * NT), nnp[it]);
  }
  // read-only step with pending sets: K_s' H' needs H and the K rows alone, so it is formed in front of the stream.  The K rows of
  // this thread's columns (c = tid, tid + NT, ...: the order of the sums) are asked for here, kFPre rounds of them; no supported
  // shape has more than three (n < 3 NT), the loops behind the rounds take what is left.
  constexpr bool kCorr = !WR && NS > 0;
  constexpr int kFPre = NS > 6 ? 2 : 3, kSPre = kFPre;       // (seven sets: three rounds of 21 registers spilled, 60 bytes of scratch)
  double kvp[kCorr ? kFPre : 1][NDA], ksp[kCorr ? kSPre : 1][NDA];
  if constexpr (kCorr) {
#pragma unroll
    for (int it = 0; it < kFPre; ++it)
      if (tid + it * NT < n) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int k = 0; k < D; ++k) kvp[it][s * D + k] = Fs[s][(size_t)(D + k) * ldx + tid + it * NT];
      }
  }
  if (tid < kPreDoubles) misc[tid] = pre_d[tid];
  constexpr bool kXlLds = !(RBPF_SYM_LIGHT_WGS > 2 && !WR && E == 0) && !kGStrip;   // three workgroups per CU: no room for the prior mean in LDS
  if (kXlLds) for (int c = tid; c < n; c += NT) xls[c] = srcX[c];
  double Riy[D];                                               // R^-1 y (:292)
  if (E > 0) {
    const double* iv = remote ? recp + a.rec_off_I : a.ivec_old + (size_t)ancb * a.ivec_old_stride;
    for (int c = tid; c < n; c += NT) Hs[c * DE + D] = iv[c];
#pragma unroll
    for (int aa = 0; aa < D; ++aa) {
      double sacc = 0.0;
#pragma unroll
      for (int bb = 0; bb < D; ++bb) sacc = fma(M.Rinv[aa + D * bb], a.y[bb], sacc);
      Riy[aa] = sacc;
    }
  }
  RBPF_SYM_KSTAMP(1);
  // ---- B: per-axis sin / cos tables (no barrier in front: nothing here reads what phase A stored) ----
  for (int q = tid; q < M.ktot; q += NT) basis_table_entry(M, q, px0, px1, px2, tabS, tabC);
  __syncthreads();
  RBPF_SYM_KSTAMP(2);
  // ---- C: measurement Jacobian, one column per thread ----
  {
    auto column = [&](int c, const int* nn) {
      double h[D];
      if (a.H_ext != nullptr) {
#pragma unroll
        for (int k = 0; k < D; ++k) h[k] = a.H_ext[((size_t)i * D + k) * ldx + c];
      } else {
        H_column<D>(M, c, nn, tabS, tabC, &misc[8], h);
      }
#pragma unroll
      for (int k = 0; k < D; ++k) Hs[c * DE + k] = h[k];
      if (E > 0) {
        double sp = Hs[c * DE + D];                               // ivecPlus = ivec + dyi'/R*yt' (:292), the new information vector (:333)
#pragma unroll
        for (int k = 0; k < D; ++k) sp = fma(h[k], Riy[k], sp);
#pragma unroll
        for (int k = 0; k < D; ++k) a.Hb_new[((size_t)i * D + k) * ldx + c] = h[k];
        a.ivec_new[(size_t)i * ldx + c] = sp;
      }
    };
#pragma unroll
    for (int it = 0; it < kNNPre; ++it)
      if (tid + it * NT < n) column(jcol(tid + it * NT), nnp[it]);
    for (int ci = tid + kNNPre * NT; ci < n; ci += NT) {
      int nn[3] = {0, 0, 0};
      if (a.H_ext == nullptr) H_column_indices(M, jcol(ci), nn);
      column(jcol(ci), nn);
    }
  }
  __syncthreads();
  if constexpr (kCorr) {
    // g = K_s' H', this wave's part: per thread over its columns in ascending order, a wave sum per value, parked in `red` (which
    // nothing touches before the cross-wave sum behind the stream; g itself does not live across the stream)
    constexpr int NG = NS * D * DE;
    double g[NG];
#pragma unroll
    for (int q = 0; q < NG; ++q) g[q] = 0.0;
    auto gcol = [&](int c, const double* kv) {
      double h[DE];
#pragma unroll
      for (int k = 0; k < DE; ++k) h[k] = Hs[c * DE + k];
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int k = 0; k < D; ++k)
#pragma unroll
          for (int j = 0; j < DE; ++j) g[(s * D + k) * DE + j] = fma(kv[s * D + k], h[j], g[(s * D + k) * DE + j]);
    };
#pragma unroll
    for (int it = 0; it < kFPre; ++it)
      if (tid + it * NT < n) gcol(tid + it * NT, kvp[it]);
    for (int c = tid + kFPre * NT; c < n; c += NT) {
      double kv[NDA];
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int k = 0; k < D; ++k) kv[s * D + k] = Fs[s][(size_t)(D + k) * ldx + c];
      gcol(c, kv);
    }
    // (four sums per register butterfly, wave_sum's totals bit for bit: no LDS round trip, no partner address to keep out of the stream)
    wave_sums_packed<NG>(g, lane, [&](int q, double s) { red[wave * kSymRed + q] = s; });
  }

  RBPF_SYM_KSTAMP(3);
  {
  // ---- D: stream the stored tiles once ----
  const int rp = (NPH == 1) ? wave : (wave % (chv / 2)), cp = (NPH == 1) ? 0 : (wave / (chv / 2));   // row pair, column phase
  const int rows[kSymRows] = {rp, chv - 1 - rp};               // ascending
  constexpr bool kQuad = RBPF_SYM_QUAD && !WR && NPH == 1 && E <= RBPF_SYM_QUAD_EMAX;   // read-only steps at CH = 8: sym_block_quad
  // wave loads in flight per quad round: runtime counts eight (sixteen spilled 4-5 registers there: 256 VGPRs; eight: 202, none)
  constexpr int kQL = CH == 0 ? 8 : RBPF_SYM_QUAD_LOADS;
  double accr[kSymRows][DE], hown[kSymRows][DE], ks[kSplit ? 1 : kSymRows][NDA];
  double accq[kQuad ? kSymRows : 1][4][DE], hq[kQuad ? kSymRows : 1][4][DE];
  if constexpr (kQuad) {
#pragma unroll
    for (int q = 0; q < kSymRows; ++q)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq)
#pragma unroll
        for (int k = 0; k < DE; ++k) { accq[q][rq][k] = 0.0; hq[q][rq][k] = Hs[(nb + rows[q] * kSymChunk + 16 * rq + (lane & 15)) * DE + k]; }
  }
#pragma unroll
  for (int q = 0; q < kSymRows; ++q) {
    const int r = nb + rows[q] * kSymChunk + lane;
#pragma unroll
    for (int k = 0; k < DE; ++k) { accr[q][k] = 0.0; hown[q][k] = Hs[r * DE + k]; }
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int k = 0; k < D; ++k) ks[kSplit ? 0 : q][s * D + k] = (WR && !kSplit) ? Fs[s][(size_t)k * ldx + r] : 0.0;
    // the border COLUMNS of this row, P(r, b) = B(b, r), downdated like the border phase does when this is a flush.  Read here,
    // before anything is stored: in the second launch of a single-bank flush the border phase overwrites these very values.
    for (int b = 0; b < nb && cp == 0 && !kQuad; ++b) {        // (once per row: the first column phase; quad mapping: after the stream)
      double pv = (double)srcB[(size_t)b * ldb + r];
      if (WR) {
#pragma unroll
        for (int sset = 0; sset < NS; ++sset)
#pragma unroll
          for (int k = 0; k < D; ++k) pv = fma(-Fs[sset][(size_t)k * ldx + b], Fs[sset][(size_t)(D + k) * ldx + r], pv);
      }
#pragma unroll
      for (int k = 0; k < DE; ++k) accr[q][k] = fma(pv, Hs[b * DE + k], accr[q][k]);
    }
  }
  if (WR) __syncthreads();                                     // every wave has read the old border block before any wave stores it
  {
    TS* dT = reinterpret_cast<TS*>(a.Pt_new) + (size_t)dslot * Ly.szT;
    double* kst = smem + lp.off_kst + (size_t)wave * kSymStage * ND;
    double* colw = (rp == 0) ? PHt + nb : (kGStrip ? smem + lp.off_col1 + (size_t)wave * DE * kSymChunk : smem + sym_off_col(lp.off_col1, DE, chv, rp));
    const int ldc = (rp == 0) ? ldx : (kGStrip ? kSymChunk : sym_ld_col(chv, rp));
    // sixteen tile rows, runtime counts: this wave's strip in the global workspace
    double* gstrip = kGStrip ? a.strip_ws + (size_t)blockIdx.x * a.strip_ws_stride + sym_off_col(0, DE, chv, rp) : nullptr;
    const double* Hcore = Hs + (size_t)nb * DE;
    // column factors K(c, .) of kSymStage columns of every pending set -> the wave's LDS stage [pair][k][e] (lane = column;
    // wave-private: program order is the only synchronisation; the fetch latency is paid once per 32 columns and hidden by the
    // other seven waves of the CU -- a register prefetch would cost 2 * ND registers across the whole stream loop)
    double kpre[NDA];
    auto fetch = [&](int col0) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int k = 0; k < D; ++k) kpre[s * D + k] = Fs[s][(size_t)(D + k) * ldx + col0 + (lane & (kSymStage - 1))];
    };
    auto park = [&]() {
      // the stage is written as doubles and read as 16-byte pairs: the compiler barriers keep the two kinds of access in program order
      // (type-based alias analysis sees them as unrelated; seen to go wrong in the one-set flush at two tile rows)
      asm volatile("" ::: "memory");
      if (lane < kSymStage) {
#pragma unroll
        for (int k = 0; k < ND; ++k) kst[((size_t)(lane >> 1) * ND + k) * 2 + (lane & 1)] = kpre[k];
      }
      asm volatile("" ::: "memory");
    };
    const int last = rows[kSymRows - 1];
    for (int J = 0; J <= last; ++J) {
      const TS* src[kSymRows]; TS* dst[kSymRows];
#pragma unroll
      for (int q = 0; q < kSymRows; ++q) {
        const size_t off = ((size_t)rows[q] * (rows[q] + 1) / 2 + J) * kSymTile + SymTile<TS>::cg * lane;
        src[q] = srcT + off; dst[q] = dT + off;
      }
      const double* Hc = Hcore + (size_t)J * kSymChunk * DE;
      double* colp = (kGStrip && rp > 0) ? colw : colw + (size_t)J * kSymChunk;
      if constexpr (kQuad) {
        const TS* srq[kSymRows];
#pragma unroll
        for (int q = 0; q < kSymRows; ++q)
          srq[q] = srcT + ((size_t)rows[q] * (rows[q] + 1) / 2 + J) * kSymTile + SymTile<TS>::cg * (kSymChunk * (lane >> 4) + (lane & 15));
        if constexpr (std::is_same<TS, float>::value) {
          if (J < rows[0]) sym_block_quad_f4<D, DE, 2, false, 0>(srq, Hc, hq, accq, colp, ldc, lane);
          else if (J == rows[0]) sym_block_quad_f4<D, DE, 2, true, 0>(srq, Hc, hq, accq, colp, ldc, lane);
          else if (J < last) sym_block_quad_f4<D, DE, 1, false, 1>(srq, Hc, hq, accq, colp, ldc, lane);
          else sym_block_quad_f4<D, DE, 1, true, 1>(srq, Hc, hq, accq, colp, ldc, lane);
        } else {
        if (J < rows[0]) sym_block_quad<TS, D, DE, 2, false, 0, kQL>(srq, Hc, hq, accq, colp, ldc, lane);
        else if (J == rows[0]) sym_block_quad<TS, D, DE, 2, true, 0, kQL>(srq, Hc, hq, accq, colp, ldc, lane);
        else if (J < last) sym_block_quad<TS, D, DE, 1, false, 1, kQL>(srq, Hc, hq, accq, colp, ldc, lane);
        else sym_block_quad<TS, D, DE, 1, true, 1, kQL>(srq, Hc, hq, accq, colp, ldc, lane);
        }
      } else if constexpr (!kSplit) {
        for (int pbeg = 0; pbeg < kSymChunk / 2; pbeg += kSymStage / 2) {
          if (WR && ND > 0) { fetch(nb + J * kSymChunk + 2 * pbeg); park(); }
          if (J < rows[0]) sym_block<TS, D, DE, NS, WR, 2, false, 0, false, kSymRows, NPH>(src, dst, Hc, kst, pbeg, cp, ks, hown, accr, colp, ldc, lane);
          else if (J == rows[0]) sym_block<TS, D, DE, NS, WR, 2, true, 0, false, kSymRows, NPH>(src, dst, Hc, kst, pbeg, cp, ks, hown, accr, colp, ldc, lane);
          else if (J < last) sym_block<TS, D, DE, NS, WR, 1, false, 1, false, kSymRows, NPH>(src, dst, Hc, kst, pbeg, cp, ks, hown, accr, colp, ldc, lane);
          else sym_block<TS, D, DE, NS, WR, 1, true, 1, false, kSymRows, NPH>(src, dst, Hc, kst, pbeg, cp, ks, hown, accr, colp, ldc, lane);
        }
      } else {
        // row 1 (always active), then row 0 where it reaches this block column; row 0's column sums are added to row 1's
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int k = 0; k < D; ++k) ks[0][s * D + k] = Fs[s][(size_t)k * ldx + nb + rows[1] * kSymChunk + lane];
        for (int pbeg = 0; pbeg < kSymChunk / 2; pbeg += kSymStage / 2) {
          fetch(nb + J * kSymChunk + 2 * pbeg); park();
          if (J < last) sym_block<TS, D, DE, NS, WR, 1, false, 1, false, 1, NPH>(src, dst, Hc, kst, pbeg, cp, ks, hown, accr, colp, ldc, lane);
          else sym_block<TS, D, DE, NS, WR, 1, true, 1, false, 1, NPH>(src, dst, Hc, kst, pbeg, cp, ks, hown, accr, colp, ldc, lane);
        }
        if (J <= rows[0]) {
#pragma unroll
          for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int k = 0; k < D; ++k) ks[0][s * D + k] = Fs[s][(size_t)k * ldx + nb + rows[0] * kSymChunk + lane];
          for (int pbeg = 0; pbeg < kSymChunk / 2; pbeg += kSymStage / 2) {
            fetch(nb + J * kSymChunk + 2 * pbeg); park();
            if (J < rows[0]) sym_block<TS, D, DE, NS, WR, 1, false, 0, true, 1, NPH>(src, dst, Hc, kst, pbeg, cp, ks, hown, accr, colp, ldc, lane);
            else sym_block<TS, D, DE, NS, WR, 1, true, 0, true, 1, NPH>(src, dst, Hc, kst, pbeg, cp, ks, hown, accr, colp, ldc, lane);
          }
        }
      }
      if (kGStrip && rp > 0 && J < last) {
        // the block column's sums leave the stage: rows k of the strip, 64 consecutive columns each (the stage is wave-private: program
        // order is the only synchronisation, as for kst)
#pragma unroll
        for (int k = 0; k < DE; ++k) gstrip[(size_t)k * sym_ld_col(chv, rp) + J * kSymChunk + lane] = colw[k * kSymChunk + lane];
      }
    }
  }
  // Behind the stream the accumulators' partners are dead: the KS rows of the correction loop and the first border columns of the quad
  // combine are asked for now, in front of the border rows, and used two barriers later.
  if constexpr (kCorr) {
    // (the thread index through an empty asm: otherwise the compiler shares these addresses with those of the K rows in the prologue
    // and keeps them across the stream -- the one-set read-only kernel at eight tile rows then spills two registers)
    int tq = tid;
    asm volatile("" : "+v"(tq));
#pragma unroll
    for (int it = 0; it < kSPre; ++it)
      if (tq + it * NT < n) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int k = 0; k < D; ++k) ksp[it][s * D + k] = Fs[s][(size_t)k * ldx + tq + it * NT];
      }
  }
  constexpr int kBPre = 4;
  double pvp[kQuad ? kSymRows : 1][kBPre];
  if constexpr (kQuad) {
#pragma unroll
    for (int q = 0; q < kSymRows; ++q)
#pragma unroll
      for (int b = 0; b < kBPre; ++b)
        if (b < nb) pvp[q][b] = (double)srcB[(size_t)b * ldb + nb + sym_quad_row(rows[q], lane)];
  }
  RBPF_SYM_KSTAMP(7);                                         // (wave 0 leaves the stream: the border rows, the combine and the correction follow)
  // border rows (row-major block B, all n columns): lanes walk columns, wave-reduce per row (as in step_kernel)
  for (int b = wave; b < nb; b += NW) {
    const TS* src = srcB + (size_t)b * ldb;
    TS* dstb = reinterpret_cast<TS*>(a.Pb_new) + (size_t)dslot * Ly.szB + (size_t)b * ldb;
    double ksb[NDA];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int k = 0; k < D; ++k) ksb[s * D + k] = WR ? Fs[s][(size_t)k * ldx + b] : 0.0;
    double accb[DE];
#pragma unroll
    for (int k = 0; k < DE; ++k) accb[k] = 0.0;
    for (int c = 2 * lane; c < ldb; c += 128) {
      const dbl2s vv = ld_tile<TS>(src + c);
      double p[2] = {vv.x, vv.y};
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int cc = c + e;
        if (cc < n) {
          if (WR) {
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
              for (int k = 0; k < D; ++k) p[e] = fma(-ksb[s * D + k], Fs[s][(size_t)(D + k) * ldx + cc], p[e]);
          }
#pragma unroll
          for (int k = 0; k < DE; ++k) accb[k] = fma(p[e], Hs[cc * DE + k], accb[k]);
        }
      }
      if (WR) { dbl2s o; o.x = p[0]; o.y = p[1]; st_tile<TS>(dstb + c, o); }
    }
    if constexpr (D > 1) {
      wave_sums_packed<DE>(accb, lane, [&](int k, double s) { PHt[(size_t)k * ldx + b] = s; });
    } else {
      // dense-radio has no border rows (nb = 0 is a condition of its launch): this loop never runs there, and with the packed form in
      // it the flushes with three and four sets took 134 and 149 registers instead of 122 and 120 (four -> three waves per SIMD)
#pragma unroll
      for (int k = 0; k < DE; ++k) {
        const double s = wave_sum(accb[k]);
        if (lane == 0) PHt[(size_t)k * ldx + b] = s;
      }
    }
  }
  if (NPH > 1 && cp > 0) {                                     // the other column phases: their row sums go through LDS
    double* rowp = smem + lp.off_row + (size_t)(cp - 1) * DE * chv * kSymChunk;
#pragma unroll
    for (int q = 0; q < kSymRows; ++q)
#pragma unroll
      for (int k = 0; k < DE; ++k) rowp[(size_t)k * (chv * kSymChunk) + rows[q] * kSymChunk + lane] = accr[q][k];
  }
  __syncthreads();
  // combine, by the lane (of the first column phase) that owns the row: row part incl. the border columns (registers) + the other
  // phase's row part + the row pairs' column parts in order
  if (cp == 0) {
#pragma unroll
    for (int q = 0; q < kSymRows; ++q) {
      // quad mapping: the four lane groups hold the row sums of rows r16 + 16 rq over their quarter of the columns; two folds add the
      // groups and leave row 16 * {0, 2, 1, 3}[lane >> 4] + r16 in this lane (wave_sum4's order), plus the border columns' part,
      // which the plain mapping accumulated for row `lane`
      const int rc = kQuad ? sym_quad_row(rows[q], lane) : rows[q] * kSymChunk + lane;   // core coordinate
      double s[DE];
#pragma unroll
      for (int k = 0; k < DE; ++k) s[k] = accr[q][k];
      if constexpr (kQuad) {
        // the border columns of this lane's row, P(r, b) = B(b, r) (not live across the stream: twelve registers for its loads)
#pragma unroll
        for (int k = 0; k < DE; ++k) s[k] = 0.0;
#pragma unroll
        for (int b = 0; b < kBPre; ++b)
          if (b < nb) {
#pragma unroll
            for (int k = 0; k < DE; ++k) s[k] = fma(pvp[q][b], Hs[b * DE + k], s[k]);
          }
        for (int b = kBPre; b < nb; ++b) {
          const double pv = (double)srcB[(size_t)b * ldb + nb + rc];
#pragma unroll
          for (int k = 0; k < DE; ++k) s[k] = fma(pv, Hs[b * DE + k], s[k]);
        }
#pragma unroll
        for (int k = 0; k < DE; ++k)
          s[k] = fold16(fold32(accq[q][0][k], accq[q][1][k]), fold32(accq[q][2][k], accq[q][3][k])) + s[k];
      }
      if (NPH > 1) {
#pragma unroll
        for (int ph = 1; ph < NPH; ++ph) {                     // phases in order: a fixed summation order
          const double* rowp = smem + lp.off_row + (size_t)(ph - 1) * DE * chv * kSymChunk;
#pragma unroll
          for (int k = 0; k < DE; ++k) s[k] += rowp[(size_t)k * (chv * kSymChunk) + rc];
        }
      }
#pragma unroll
      for (int w = 0; w < chv / 2; ++w) {
        if (rows[q] < chv - 1 - w) {                          // row pair w holds off-diagonal tiles in this block column
          const double* cw = (w == 0) ? PHt + nb : (kGStrip ? a.strip_ws + (size_t)blockIdx.x * a.strip_ws_stride + sym_off_col(0, DE, chv, w)
                                                            : smem + sym_off_col(lp.off_col1, DE, chv, w));
          const int ldw = (w == 0) ? ldx : sym_ld_col(chv, w);
#pragma unroll
          for (int k = 0; k < DE; ++k) s[k] += cw[(size_t)k * ldw + rc];
        }
      }
#pragma unroll
      for (int k = 0; k < DE; ++k) PHt[(size_t)k * ldx + nb + rc] = s[k];
    }
  }
  __syncthreads();
  }
  if (!WR && NS > 0) {
    // read-only step: PHt holds P_base * H'; subtract sum_s KS_s * (K_s' * H')
    // (the waves' parts of g = K_s' H' have lain in `red` since the prologue; they are added here in wave order)
    constexpr int NG = NS * D * DE > 0 ? NS * D * DE : 1;
    double g[NG];
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      double s = red[q];
      for (int w = 1; w < NW; ++w) s += red[w * kSymRed + q];
      g[q] = s;
    }
    auto corr = [&](int r, const double* ksr) {
      double ph[DE];
#pragma unroll
      for (int j = 0; j < DE; ++j) ph[j] = PHt[(size_t)j * ldx + r];
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int k = 0; k < D; ++k)
#pragma unroll
          for (int j = 0; j < DE; ++j) ph[j] = fma(-ksr[s * D + k], g[(s * D + k) * DE + j], ph[j]);
#pragma unroll
      for (int j = 0; j < DE; ++j) PHt[(size_t)j * ldx + r] = ph[j];
    };
#pragma unroll
    for (int it = 0; it < kSPre; ++it)
      if (tid + it * NT < n) corr(tid + it * NT, ksp[kCorr ? it : 0]);
    int tq = tid;
    asm volatile("" : "+v"(tq));                               // (as above)
    for (int r = tq + kSPre * NT; r < n; r += NT) {
      double ksr[NDA];
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int k = 0; k < D; ++k) ksr[s * D + k] = Fs[s][(size_t)k * ldx + r];
      corr(r, ksr);
    }
    __syncthreads();
  }

  RBPF_SYM_KSTAMP(4);
  // ---- E: S = H (P H') + R, e = y - H xl   (particleFilter.m:139-150) ----
  constexpr int NRED = D * D + D + 2 * E;
  {
    double part[NRED];
#pragma unroll
    for (int q = 0; q < NRED; ++q) part[q] = 0.0;
    for (int r = tid; r < n; r += NT) {
      double h[D], ph[D];
#pragma unroll
      for (int k = 0; k < D; ++k) { h[k] = Hs[r * DE + k]; ph[k] = PHt[(size_t)k * ldx + r]; }
      const double x = kXlLds ? xls[r] : srcX[r];
#pragma unroll
      for (int bb = 0; bb < D; ++bb)
#pragma unroll
        for (int aa = 0; aa < D; ++aa) part[aa + D * bb] = fma(h[aa], ph[bb], part[aa + D * bb]);
#pragma unroll
      for (int aa = 0; aa < D; ++aa) part[D * D + aa] = fma(h[aa], x, part[D * D + aa]);
      if (E > 0) {
        // ivec' P ivec and ivecPlus' P ivecPlus (:301-303), P = the (downdated) prior covariance
        const double iv = Hs[r * DE + D], piv = PHt[(size_t)D * ldx + r];
        double ivp = iv, pivp = piv;
#pragma unroll
        for (int k = 0; k < D; ++k) { ivp = fma(h[k], Riy[k], ivp); pivp = fma(ph[k], Riy[k], pivp); }
        part[D * D + D] = fma(iv, piv, part[D * D + D]);
        part[D * D + D + 1] = fma(ivp, pivp, part[D * D + D + 1]);
      }
    }
    wave_sums_packed<NRED>(part, lane, [&](int q, double s) { red[wave * kSymRed + q] = s; });
  }
  __syncthreads();
  if (wave == 0) {
    // Lane q < NRED adds value q over the waves, in wave order; lane reads then hand every sum to every lane, and the lanes of the
    // wave run the factorisation side by side on the same numbers (one lane stores).  The D logarithms are one call: lane q takes
    // cS(q, q).  Each expression is the one a single lane evaluated before.
    double sq = 0.0;
    if (lane < NRED) {
      sq = red[lane];
      for (int w = 1; w < NW; ++w) sq += red[w * kSymRed + lane];
    }
    double SS[D * D], e[D], cS[D * D] = {}, v[D];                           // (cS: a failed factorisation leaves part of it unwritten)
#pragma unroll
    for (int q = 0; q < D * D; ++q) SS[q] = sym_lane_read(sq, q) + M.R[q];    // particleFilter.m:141
#pragma unroll
    for (int q = 0; q < D; ++q) e[q] = a.y[q] - sym_lane_read(sq, D * D + q); // :140
    bool ok = chol_lower_small<D>(SS, cS);                                  // :145
    if (!ok) {
      double SJ[D * D];
      for (int q = 0; q < D * D; ++q) SJ[q] = SS[q];
      for (int q = 0; q < D; ++q) SJ[q + D * q] += M.jitter;                // :147
      ok = chol_lower_small<D>(SJ, cS);
    }
    double dg = cS[0];
#pragma unroll
    for (int q = 1; q < D; ++q) dg = (lane == q) ? cS[q + D * q] : dg;
    const double lg = log(dg);                                              // (of whatever a failed factorisation left: not used then)
    double lgq[D];
#pragma unroll
    for (int q = 0; q < D; ++q) lgq[q] = sym_lane_read(lg, q);
    double lw = 0.0, sl = 0.0;
    if (ok) {
      fwd_subst<D>(cS, e, v);                                               // :149
      double vv = 0.0;
      for (int q = 0; q < D; ++q) { sl += lgq[q]; vv += v[q] * v[q]; }
      lw = -sl - 0.5 * vv + M.logconst;                                     // :150
    } else {
      lw = nan("");
      for (int q = 0; q < D * D; ++q) cS[q] = 0.0;
      for (int q = 0; q < D; ++q) cS[q + D * q] = 1.0;
    }
    if (lane == 0) {
      if (!ok) atomicOr(a.status, 1);
      if (E == 0) a.logw[i] = lw;
      for (int q = 0; q < D * D; ++q) { misc[20 + q] = cS[q]; misc[30 + q] = SS[q]; }
      for (int q = 0; q < D; ++q) misc[40 + q] = e[q];
    }
    if (E > 0) {
      const double qa = sym_lane_read(sq, D * D + D), qb = sym_lane_read(sq, D * D + D + 1);
      if (lane == 0) { misc[44] = qa; misc[45] = qb; misc[46] = ok ? sl : nan(""); }   // sl: the sum of the logarithms, in order
    }
  }
  __syncthreads();

  RBPF_SYM_KSTAMP(5);
  // ---- F: Kalman gain rows, mean update, new pending factors (particleFilter.m:194-198) ----
  {
    double cS[D * D], SS[D * D], e[D];
#pragma unroll
    for (int q = 0; q < D * D; ++q) { cS[q] = misc[20 + q]; SS[q] = misc[30 + q]; }
#pragma unroll
    for (int q = 0; q < D; ++q) e[q] = misc[40 + q];
    double* KSn = a.F_new + ((size_t)i * 2 + 0) * D * ldx;
    double* Kn = a.F_new + ((size_t)i * 2 + 1) * D * ldx;
    if (tid == 0) {
      if (a.base_new) a.base_new[i] = WR ? dslot : (a.share_flush ? pre_i[4] : baseb);
      if (!WR) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
          if (a.fset_idx_new[s]) a.fset_idx_new[s][i] = pre_i[kPreSet0 + s];
      }
      if (a.fself_idx_new) a.fself_idx_new[i] = i;
    }
    double* xln = a.xl_new + (size_t)i * ldx;
    double uK[D];
#pragma unroll
    for (int k = 0; k < D; ++k) uK[k] = 0.0;
    for (int r = tid; r < n; r += NT) {
      double ph[D], u[D], kk[D];
#pragma unroll
      for (int k = 0; k < D; ++k) ph[k] = PHt[(size_t)k * ldx + r];
      fwd_subst<D>(cS, ph, u);
      bwd_subst_T<D>(cS, u, kk);
      double xn_ = kXlLds ? xls[r] : srcX[r];
#pragma unroll
      for (int k = 0; k < D; ++k) xn_ = fma(kk[k], e[k], xn_);              // :197
      xln[r] = xn_;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) s = fma(kk[k], SS[k + D * j], s);
        KSn[(size_t)j * ldx + r] = s;
        Kn[(size_t)j * ldx + r] = kk[j];
      }
      if (E > 0) {
        double ivp = Hs[r * DE + D];
#pragma unroll
        for (int k = 0; k < D; ++k) ivp = fma(Hs[r * DE + k], Riy[k], ivp);
#pragma unroll
        for (int k = 0; k < D; ++k) uK[k] = fma(ivp, kk[k], uK[k]);            // ivecPlus' * K
      }
    }
    if (E > 0) {
      __syncthreads();
      wave_sums_packed<D>(uK, lane, [&](int k, double s) { red[wave * kSymRed + k] = s; });
      __syncthreads();
      if (tid == 0) {
        double u[D];
        for (int k = 0; k < D; ++k) { double s = red[k]; for (int w = 1; w < NW; ++w) s += red[w * kSymRed + k]; u[k] = s; }
        double corr = 0.0;                                                  // ivecPlus' * (K*SS*K') * ivecPlus
        for (int bb = 0; bb < D; ++bb) {
          double t = 0.0;
          for (int aa = 0; aa < D; ++aa) t = fma(u[aa], SS[aa + D * bb], t);
          corr = fma(t, u[bb], corr);
        }
        const double qa = misc[44], qbp = misc[45] - corr, sl = misc[46];
        const double hld = remote ? recp[a.rec_off_hld] : a.hld_old[(size_t)ancb * a.hld_old_stride];
        const double hldp = -sl + M.halfLogDetR + hld;                       // :298
        double yRy = 0.0;
        for (int bb = 0; bb < D; ++bb) {
          double t = 0.0;
          for (int aa = 0; aa < D; ++aa) t = fma(a.y[aa], M.Rinv[aa + D * bb], t);
          yRy = fma(t, a.y[bb], yRy);
        }
        // :301-304   (1/2*log((2*pi)^ny*det(R)) = -logconst + halfLogDetR)
        a.logw[i] = -0.5 * qa - hld + hldp + 0.5 * qbp - 0.5 * yRy - (-M.logconst + M.halfLogDetR);
        a.hld_new[i] = hldp;
        a.qf_new[i] = qbp;
      }
    }
  }
  RBPF_SYM_KSTAMP(6);
