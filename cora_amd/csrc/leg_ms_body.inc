// leg_ms_body.inc - one macro-step (8 consecutive l, 16 MFMAs in the <8,1> shape) of legendre_kernel's stage loop.
// LEG_CLEAN: 1 steady-state stages (no tests at all), 2 head stages whose rows all exist (unrolled like the steady-state
// ones, fast refill pieces, but rings of the wave may still enter: the wave-uniform skip tests and the entry select
// stay), 0 the rolled generic form (tail stages, and heads of items too short for the fast pieces).
// LEG_MS is the macro-step index inside the stage: a LITERAL in the steady-state (LEG_CLEAN) stages - the body is
// included LEG_KT / 8 times, so that every LDS offset and the LDS-DMA destination of the refill piece are immediates -
// and the loop variable in the rolled head / tail stages.  `continue` leaves the macro-step in both forms (the textual
// copies sit in do { } while (0)).
                    // one a_lm piece of the stage being refilled per macro-step: spreads the LDS-DMA issue
                    // over the MFMA work instead of an 8-wave burst behind the barrier (measured 7 % of time)
#if LEG_CLEAN
                    issue_row_fast(rsrc, rdst, std::integral_constant<int, LEG_MS * LEG_RPM>{});
#if LEG_RPM > 1
                    issue_row_fast(rsrc, rdst, std::integral_constant<int, LEG_MS * LEG_RPM + 1>{});
#endif
#if LEG_RPM > 2
#error "leg_ms_body.inc: more than two a_lm pieces per macro-step"
#endif
#else
                    if (refill) {
#pragma unroll
                        for (int r = 0; r < RPM; r++) issue_row(w, st + LEG_NBUF - 1, LEG_MS * RPM + r);
                    }
#endif
                    const int l0 = ls + 8 * LEG_MS;
                    if (!LEG_CLEAN && l0 > lmax) continue;
                    // nothing of this wave starts before l0+14: skip the macro-step entirely
                    if (LEG_CLEAN != 1 && ws_min > l0 + 13) continue;
                    double ae[RT], ao[RT];
                    double2 c[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) c[j] = sc[8 * LEG_MS + j];
                    if (LEG_CLEAN != 1 && ws_maxinj >= l0) {   // (scalar) some ring of the wave may still enter at or after this macro-step
                        const int lf = l0 + d;             // entry rows are window starts of the lane (plan: d_seed4)
#pragma unroll
                        for (int q = 0; q < RT; q++) {
                            const bool inj = (inj_l[q] == lf);
                            p0[q] = inj ? sd[q].x : p0[q];
                            p1[q] = inj ? sd[q].y : p1[q];
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 8; j++) {
#pragma unroll
                        for (int q = 0; q < RT; q++) {
                            const double vv = fma(c[j].x * x[q], p1[q], -p0[q]);
                            p0[q] = p1[q];
                            p1[q] = vv;
                            if (j == 0) ae[q] = vv * c[0].y;      // lambda = s mu
                            if (j == 1) ao[q] = vv * c[1].y;
                        }
                    }
                    if (LEG_CLEAN != 1 && ws_min > l0 + 7) continue;  // all A operands of this macro-step are zero
#if LEG_STAMPS && !LEG_CLEAN
                    n_tail_ms++;
#endif
                    const double *be = sb + (8 * LEG_MS + d) * STRIDE + ri;
                    const double *bo = be + STRIDE;
#pragma unroll
                    for (int t = 0; t < NT; t++) {
                        const double bev = be[16 * t], bov = bo[16 * t];
#pragma unroll
                        for (int q = 0; q < RT; q++) {
                            acce[q][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ae[q], bev, acce[q][t], 0, 0, 0);
                            acco[q][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ao[q], bov, acco[q][t], 0, 0, 0);
                        }
                    }
