"""The general AbbyNormal row kernels (csrc/abby.hip: abby_fwd_kernel<E> / abby_bwd_kernel<E> at d = 128 ... 1024,
abby_fwd64_kernel / abby_bwd64_kernel at d = 64) against the float64 reference of tests/abby_ref.py, through the
C entry points, every output filled with ref_check.SENTINEL first.  Reference, inputs, metric (per row, bound =
max(floor, 20 e32), e32 the reference's own float32 evaluation), exclusions and their cap are described there;
tests/test_abby_ref.py proves on the CPU that the bounds are honest and that every listed mutation breaks them.

d in {64, 128, 256, 384, 512, 768, 1024} -- every case of the dispatch switches, the backward's AHEAD == 1 loop at
768 and 1024 -- at 1, 3, 4, 5 and 74 rows, and at the row counts of abby_ref.FWD_WRAP / BWD_WRAP that wrap the
grid-stride loops and end ragged in their second and first arm (tests/test_abby_ref.py derives that from the grid
caps).  Forward: asrx_abby_fwd_logits2 (controlled modes r % 3; ties tier with mode 2 on every row), asrx_abby_fwd2
(hpre / W2), asrx_abby_fwd3 with nrm and asrx_abby_fwd_res on both forms, asrx_abby_fwd2 with tw / tb / tc, fp32
and bf16 out (the bf16 out is the fp32 out rounded, bit for bit; ys, idx, tc equal), keyed noise at H in {1, 3}.
Backward: asrx_abby_bwd2 on the reference's own ys (rounded to fp32) and idx, mixed tier with modes r % 3 and ties
tier with mode 2 everywhere, acc = 0 and acc = 1 into a random old dx, dW2 / db2 zeroed before each call.

Figures measured on an MI355X when these tests were added.  One line per kernel, d and row count: of every
comparison of that output there (entry points, forms, tiers, fp32 / acc variants; the noise cases are the rows 74 H),
the one with the largest e / bound.  e and e32 are the per-row metric of abby_ref.py (ys absolute, dW2 / db2 relative
to their largest entry), bound = max(floor, 20 e32); `edge` is part of out and not listed, dhpre0 is named below.  fwd64 / bwd64 are
abby_fwd64_kernel / abby_bwd64_kernel.

  kernel d    rows  out: e / e32 / bound     ys: e / e32 / bound      nrm: e / e32 / bound     tc: e / e32 / bound
  fwd64  64   1     8.1e-08/1.0e-07/1.0e-05  4.3e-08/1.0e-07/1.0e-05  --                       --
  fwd64  64   3     7.9e-08/5.7e-08/1.0e-05  4.7e-08/7.2e-08/1.0e-05  --                       --
  fwd64  64   4     8.2e-08/5.9e-08/1.0e-05  5.6e-08/5.6e-08/1.0e-05  --                       --
  fwd64  64   5     8.3e-08/9.7e-08/1.0e-05  1.6e-07/9.9e-08/1.0e-05  --                       --
  fwd64  64   74    2.5e-07/1.4e-07/1.0e-05  1.8e-07/1.2e-07/1.0e-05  --                       --
  fwd64  64   222   3.5e-07/1.6e-07/1.0e-05  2.2e-07/1.7e-07/1.0e-05  --                       --
  fwd    128  1     1.6e-07/1.1e-07/1.0e-05  3.9e-08/2.1e-08/1.0e-05  2.0e-08/4.3e-08/1.0e-05  7.4e-08/5.9e-08/1.0e-05
  fwd    128  3     9.0e-08/1.2e-07/1.0e-05  6.3e-08/3.5e-08/1.0e-05  1.4e-08/1.4e-08/1.0e-05  7.0e-08/7.7e-08/1.0e-05
  fwd    128  4     9.7e-08/6.6e-08/1.0e-05  7.6e-08/9.5e-08/1.0e-05  2.8e-08/3.4e-08/1.0e-05  1.1e-07/2.8e-07/1.0e-05
  fwd    128  5     1.1e-07/1.1e-07/1.0e-05  1.0e-07/5.2e-08/1.0e-05  3.7e-08/5.4e-08/1.0e-05  2.4e-07/2.6e-07/1.0e-05
  fwd    128  74    2.4e-07/2.1e-07/1.0e-05  3.8e-07/2.5e-07/1.0e-05  8.1e-08/1.2e-07/1.0e-05  7.1e-07/7.7e-07/1.6e-05
  fwd    128  222   2.5e-07/1.6e-07/1.0e-05  2.2e-07/2.5e-07/1.0e-05  --                       --
  fwd    128  16387 3.8e-07/2.2e-07/1.0e-05  3.8e-07/4.8e-07/1.0e-05  1.2e-07/1.4e-07/1.0e-05  --
  fwd    128  32773 4.2e-07/2.0e-07/1.0e-05  3.8e-07/4.1e-07/1.0e-05  1.1e-07/1.5e-07/1.0e-05  --
  fwd    256  1     1.1e-07/1.0e-07/1.0e-05  4.2e-08/4.2e-08/1.0e-05  1.1e-08/5.7e-08/1.0e-05  2.1e-07/1.5e-07/1.0e-05
  fwd    256  3     1.1e-07/1.1e-07/1.0e-05  8.9e-08/8.9e-08/1.0e-05  3.5e-08/3.5e-08/1.0e-05  4.5e-07/6.8e-07/1.4e-05
  fwd    256  4     1.0e-07/1.1e-07/1.0e-05  1.7e-07/1.1e-07/1.0e-05  1.4e-08/6.9e-08/1.0e-05  1.0e-07/1.0e-07/1.0e-05
  fwd    256  5     1.2e-07/1.2e-07/1.0e-05  5.9e-08/1.9e-07/1.0e-05  5.9e-08/7.4e-08/1.0e-05  3.2e-07/2.8e-07/1.0e-05
  fwd    256  74    2.0e-07/1.8e-07/1.0e-05  1.9e-07/3.8e-07/1.0e-05  7.1e-08/1.1e-07/1.0e-05  6.5e-07/6.5e-07/1.3e-05
  fwd    384  1     9.7e-08/1.2e-07/1.0e-05  3.2e-08/3.2e-08/1.0e-05  1.6e-08/1.6e-08/1.0e-05  1.4e-07/4.3e-07/1.0e-05
  fwd    384  3     1.4e-07/8.9e-08/1.0e-05  4.8e-07/2.5e-07/1.0e-05  3.1e-08/3.2e-08/1.0e-05  3.0e-07/6.6e-07/1.3e-05
  fwd    384  4     1.0e-07/1.2e-07/1.0e-05  2.2e-07/2.7e-07/1.0e-05  2.2e-08/4.6e-08/1.0e-05  1.4e-07/2.4e-07/1.0e-05
  fwd    384  5     2.3e-07/1.3e-07/1.0e-05  9.1e-08/1.3e-07/1.0e-05  5.0e-08/5.0e-08/1.0e-05  3.1e-07/4.0e-07/1.0e-05
  fwd    384  74    3.6e-07/1.7e-07/1.0e-05  2.6e-07/4.7e-07/1.0e-05  8.6e-08/9.9e-08/1.0e-05  5.8e-07/9.5e-07/1.9e-05
  fwd    384  16387 4.4e-07/2.5e-07/1.0e-05  5.2e-07/8.4e-07/1.7e-05  1.2e-07/1.4e-07/1.0e-05  --
  fwd    512  1     1.2e-07/1.3e-07/1.0e-05  2.5e-08/2.5e-08/1.0e-05  3.2e-08/3.2e-08/1.0e-05  1.1e-07/1.1e-07/1.0e-05
  fwd    512  3     2.3e-07/1.6e-07/1.0e-05  6.2e-08/3.3e-08/1.0e-05  3.4e-08/3.4e-08/1.0e-05  7.8e-08/3.6e-07/1.0e-05
  fwd    512  4     1.2e-07/1.0e-07/1.0e-05  2.9e-07/4.5e-07/1.0e-05  3.4e-08/2.7e-08/1.0e-05  1.2e-07/3.4e-07/1.0e-05
  fwd    512  5     2.7e-07/1.8e-07/1.0e-05  1.2e-07/2.7e-07/1.0e-05  4.9e-08/4.9e-08/1.0e-05  2.3e-07/2.8e-07/1.0e-05
  fwd    512  74    2.7e-07/1.8e-07/1.0e-05  3.7e-07/7.4e-07/1.5e-05  6.2e-08/1.1e-07/1.0e-05  4.1e-07/8.7e-07/1.7e-05
  fwd    768  1     1.2e-07/8.0e-08/1.0e-05  3.5e-08/3.5e-08/1.0e-05  3.1e-08/3.1e-08/1.0e-05  2.2e-07/2.3e-07/1.0e-05
  fwd    768  3     1.6e-07/1.4e-07/1.0e-05  1.7e-07/2.5e-07/1.0e-05  5.0e-08/5.0e-08/1.0e-05  3.2e-07/4.2e-07/1.0e-05
  fwd    768  4     1.7e-07/1.5e-07/1.0e-05  1.5e-07/1.9e-07/1.0e-05  3.6e-08/3.6e-08/1.0e-05  2.0e-07/4.0e-07/1.0e-05
  fwd    768  5     2.1e-07/2.1e-07/1.0e-05  1.7e-07/4.1e-07/1.0e-05  3.3e-08/3.3e-08/1.0e-05  1.0e-06/8.7e-07/1.7e-05
  fwd    768  74    3.1e-07/2.1e-07/1.0e-05  4.1e-07/8.1e-07/1.6e-05  7.7e-08/1.0e-07/1.0e-05  2.6e-06/2.1e-06/4.2e-05
  fwd    768  222   3.8e-07/2.4e-07/1.0e-05  5.0e-07/8.6e-07/1.7e-05  --                       --
  fwd    1024 1     1.1e-07/1.3e-07/1.0e-05  1.9e-08/1.9e-08/1.0e-05  2.6e-08/2.6e-08/1.0e-05  6.2e-08/1.4e-07/1.0e-05
  fwd    1024 3     1.1e-07/1.3e-07/1.0e-05  2.9e-07/2.0e-07/1.0e-05  1.8e-08/1.8e-08/1.0e-05  1.8e-07/3.0e-07/1.0e-05
  fwd    1024 4     1.3e-07/1.3e-07/1.0e-05  7.5e-08/2.0e-07/1.0e-05  3.9e-08/6.4e-08/1.0e-05  1.1e-07/2.7e-07/1.0e-05
  fwd    1024 5     1.8e-07/1.8e-07/1.0e-05  2.2e-07/2.8e-07/1.0e-05  4.6e-08/6.8e-08/1.0e-05  2.0e-07/3.2e-07/1.0e-05
  fwd    1024 74    3.5e-07/2.2e-07/1.0e-05  4.1e-07/9.2e-07/1.8e-05  8.8e-08/1.1e-07/1.0e-05  4.4e-07/9.7e-07/1.9e-05
  kernel d    rows  dx: e / e32 / bound      dhpre: e / e32 / bound   dW2: e / e32 / bound     db2: e / e32 / bound
  bwd64  64   1     8.9e-08/8.4e-08/1.0e-04  3.0e-04/2.5e-04/5.0e-03  3.8e-04/3.8e-04/7.6e-03  3.8e-04/3.8e-04/7.6e-03
  bwd64  64   3     9.1e-08/1.0e-07/1.0e-04  7.8e-07/7.3e-07/1.0e-04  7.2e-07/6.7e-07/1.0e-04  8.9e-07/8.5e-07/1.0e-04
  bwd64  64   4     1.5e-07/1.1e-07/1.0e-04  1.2e-05/1.1e-05/2.2e-04  7.7e-07/2.2e-07/1.0e-04  2.3e-06/4.6e-07/1.0e-04
  bwd64  64   5     9.2e-08/1.4e-07/1.0e-04  6.0e-06/1.6e-05/3.2e-04  5.3e-07/1.5e-06/1.0e-04  1.1e-06/1.6e-06/1.0e-04
  bwd64  64   74    3.2e-07/2.2e-07/1.0e-04  2.5e-05/2.1e-05/4.3e-04  6.6e-07/6.6e-07/1.0e-04  4.5e-07/1.9e-07/1.0e-04
  bwd64  64   16389 6.7e-07/4.1e-07/1.0e-04  2.6e-03/1.3e-03/2.7e-02  1.1e-06/2.5e-06/1.0e-04  7.2e-06/1.4e-05/2.9e-04
  bwd    128  1     9.7e-08/9.3e-08/1.0e-04  6.5e-07/5.5e-07/1.0e-04  5.8e-07/5.8e-07/1.0e-04  5.8e-07/5.8e-07/1.0e-04
  bwd    128  3     1.1e-07/9.9e-08/1.0e-04  3.0e-07/3.8e-07/1.0e-04  2.0e-07/2.1e-07/1.0e-04  1.4e-07/1.2e-07/1.0e-04
  bwd    128  4     1.1e-07/1.1e-07/1.0e-04  2.5e-07/4.3e-07/1.0e-04  2.1e-07/5.8e-07/1.0e-04  2.4e-07/4.0e-07/1.0e-04
  bwd    128  5     1.2e-07/1.1e-07/1.0e-04  1.0e-06/1.2e-06/1.0e-04  2.7e-07/2.7e-07/1.0e-04  1.6e-07/4.0e-07/1.0e-04
  bwd    128  74    2.0e-07/2.0e-07/1.0e-04  1.4e-05/1.4e-05/2.8e-04  2.9e-07/3.4e-07/1.0e-04  6.1e-07/1.1e-06/1.0e-04
  bwd    128  4099  3.3e-07/2.4e-07/1.0e-04  4.5e-03/3.2e-03/6.4e-02  1.3e-06/2.0e-06/1.0e-04  9.6e-07/4.7e-08/1.0e-04
  bwd    128  8197  3.8e-07/3.5e-07/1.0e-04  9.7e-03/3.4e-03/6.7e-02  8.0e-07/2.1e-06/1.0e-04  3.9e-07/1.8e-07/1.0e-04
  bwd    256  1     9.2e-08/9.9e-08/1.0e-04  2.0e-07/4.1e-07/1.0e-04  2.3e-07/1.9e-07/1.0e-04  1.9e-07/4.4e-07/1.0e-04
  bwd    256  3     1.1e-07/1.1e-07/1.0e-04  3.1e-06/1.3e-06/1.0e-04  5.1e-07/4.9e-07/1.0e-04  5.1e-07/4.2e-07/1.0e-04
  bwd    256  4     1.1e-07/1.1e-07/1.0e-04  1.8e-06/2.1e-06/1.0e-04  1.4e-06/1.7e-06/1.0e-04  1.2e-06/1.5e-06/1.0e-04
  bwd    256  5     2.0e-07/2.0e-07/1.0e-04  3.4e-06/5.1e-06/1.0e-04  2.4e-07/6.4e-07/1.0e-04  2.0e-06/5.3e-06/1.1e-04
  bwd    256  74    2.0e-07/2.1e-07/1.0e-04  1.0e-05/1.1e-05/2.2e-04  5.5e-07/5.8e-07/1.0e-04  1.5e-06/8.0e-07/1.0e-04
  bwd    384  1     9.6e-08/8.3e-08/1.0e-04  2.5e-07/4.8e-07/1.0e-04  1.9e-07/3.4e-07/1.0e-04  1.9e-07/3.6e-07/1.0e-04
  bwd    384  3     9.5e-08/1.0e-07/1.0e-04  5.0e-07/7.0e-07/1.0e-04  4.1e-07/9.3e-07/1.0e-04  4.7e-06/1.2e-05/2.4e-04
  bwd    384  4     1.0e-07/1.5e-07/1.0e-04  8.4e-07/2.8e-06/1.0e-04  2.3e-07/3.2e-07/1.0e-04  3.1e-06/3.0e-06/1.0e-04
  bwd    384  5     1.4e-07/1.1e-07/1.0e-04  1.5e-06/2.4e-06/1.0e-04  1.5e-07/3.0e-07/1.0e-04  1.0e-07/2.9e-07/1.0e-04
  bwd    384  74    2.1e-07/2.3e-07/1.0e-04  2.8e-05/9.4e-05/1.9e-03  3.5e-07/6.6e-07/1.0e-04  5.7e-07/1.2e-06/1.0e-04
  bwd    384  4099  6.3e-07/2.6e-07/1.0e-04  4.7e-04/8.7e-04/1.7e-02  9.0e-07/2.2e-06/1.0e-04  9.9e-07/1.4e-06/1.0e-04
  bwd    384  8197  4.7e-07/2.7e-07/1.0e-04  1.6e-03/1.8e-03/3.6e-02  1.4e-06/2.5e-06/1.0e-04  9.8e-07/4.8e-07/1.0e-04
  bwd    512  1     9.0e-08/1.7e-07/1.0e-04  6.2e-07/4.1e-07/1.0e-04  8.8e-07/1.3e-06/1.0e-04  8.2e-07/1.3e-06/1.0e-04
  bwd    512  3     1.8e-07/1.6e-07/1.0e-04  9.8e-06/1.0e-05/2.0e-04  9.5e-06/1.2e-05/2.4e-04  9.5e-06/1.2e-05/2.4e-04
  bwd    512  4     1.3e-07/1.2e-07/1.0e-04  8.3e-07/1.8e-06/1.0e-04  5.1e-07/9.1e-07/1.0e-04  5.2e-07/2.6e-06/1.0e-04
  bwd    512  5     2.2e-07/1.4e-07/1.0e-04  8.6e-07/5.8e-07/1.0e-04  3.2e-07/2.8e-07/1.0e-04  1.9e-07/8.7e-08/1.0e-04
  bwd    512  74    2.2e-07/1.8e-07/1.0e-04  8.9e-05/5.8e-05/1.2e-03  5.5e-07/6.3e-07/1.0e-04  1.3e-06/1.6e-06/1.0e-04
  bwd    768  1     1.2e-07/1.3e-07/1.0e-04  2.5e-07/1.0e-06/1.0e-04  2.4e-07/1.0e-06/1.0e-04  1.4e-07/1.1e-06/1.0e-04
  bwd    768  3     1.4e-07/1.1e-07/1.0e-04  7.1e-07/1.1e-06/1.0e-04  6.0e-07/9.7e-07/1.0e-04  5.4e-07/1.0e-06/1.0e-04
  bwd    768  4     2.5e-07/1.5e-07/1.0e-04  8.6e-07/1.4e-06/1.0e-04  4.1e-07/4.1e-07/1.0e-04  2.9e-07/2.9e-07/1.0e-04
  bwd    768  5     1.4e-07/1.9e-07/1.0e-04  2.9e-06/1.1e-05/2.3e-04  2.5e-07/4.3e-07/1.0e-04  6.5e-07/1.7e-06/1.0e-04
  bwd    768  74    2.9e-07/2.9e-07/1.0e-04  9.9e-06/3.3e-05/6.5e-04  3.3e-07/3.3e-07/1.0e-04  3.7e-07/1.9e-07/1.0e-04
  bwd    768  4099  4.4e-07/3.3e-07/1.0e-04  2.7e-03/2.2e-03/4.5e-02  9.8e-07/2.0e-06/1.0e-04  1.3e-06/1.9e-06/1.0e-04
  bwd    1024 1     1.8e-07/7.1e-08/1.0e-04  2.0e-07/4.8e-07/1.0e-04  1.6e-07/3.5e-07/1.0e-04  1.4e-07/3.1e-07/1.0e-04
  bwd    1024 3     1.2e-07/1.5e-07/1.0e-04  1.1e-06/9.7e-07/1.0e-04  2.0e-07/9.1e-07/1.0e-04  3.8e-07/3.5e-06/1.0e-04
  bwd    1024 4     1.4e-07/8.4e-08/1.0e-04  4.8e-07/1.5e-06/1.0e-04  6.9e-07/1.5e-06/1.0e-04  6.8e-07/1.6e-06/1.0e-04
  bwd    1024 5     1.7e-07/1.6e-07/1.0e-04  2.7e-06/2.4e-06/1.0e-04  4.4e-07/4.8e-07/1.0e-04  3.8e-07/3.9e-07/1.0e-04
  bwd    1024 74    2.5e-07/1.8e-07/1.0e-04  7.7e-05/7.8e-05/1.6e-03  4.9e-07/2.0e-06/1.0e-04  3.4e-07/3.6e-07/1.0e-04
  bwd    1024 4099  5.2e-07/3.4e-07/1.0e-04  8.0e-04/7.2e-04/1.4e-02  1.2e-06/1.8e-06/1.0e-04  9.5e-07/9.5e-07/1.0e-04

The largest e / bound of the 1875 comparisons is 0.14 (dhpre of the ties tier at d = 128, 8197 rows: e = 9.7e-03 on the
row whose dz cancels most, where the reference's own float32 evaluation is off by 3.4e-03); the largest outside
dhpre is 0.06 (tc of asrx_abby_fwd_logits2 at d = 768, 74 rows).  dhpre0, the absolute error on the dead rows of
abby_ref.py (exact dhpre 0), is 2.3e-05 at most (mixed tier, d = 64, 16389 rows; float32 evaluation 3.7e-05).  No
exclusion cap was exceeded: one row of 74 at most (1.4 %), 0.05 % to 0.4 % of the rows at the forward's wrap sizes,
0.3 % to 1.3 % at the backward's, where a close max-against-2-avg decision on any row counts.  dW2 / db2 arrive through
atomics, so their figures move a little from run to run.
"""
import types

import pytest
import torch

import abby_ref as A
from ref_check import SENTINEL, dev, sentinel
from ref_check import call as _call

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
KEY, SID = 0x5EED1234, 3


def _id(c):
    return "-".join(str(v) for v in c)


def _buf(rows, d, bf16=0):
    return torch.full((rows, d), SENTINEL, device="cuda", dtype=BF16 if bf16 else torch.float32)


_DEV = {}


def _devs(t):
    """The case's operands on the device, made once per case (one case is alive at a time)."""
    k = (t.tier, t.d, t.rows)
    if k not in _DEV:
        _DEV.clear()
        _DEV[k] = types.SimpleNamespace(**{n: dev(getattr(t, n)) for n in
                                           ("x", "b2", "logits", "hpre", "W2", "res", "tw", "tb", "old")})
    return _DEV[k]


def _fwd(entry, t, form, *, bf16=0, tw=False, nrm=False, noise=0, L=None, H=1, key=KEY):
    """One forward launch; returns out / ys / idx / nrm / tc (None where the entry point has none)."""
    g = _devs(t)
    rows, d = t.rows, t.d
    L = rows if L is None else L
    out, ys = _buf(rows, d, bf16), sentinel(rows, 3)
    idx = torch.full((rows,), 7, dtype=torch.int32, device="cuda")
    tc = sentinel(rows, 3) if tw else None
    nv = sentinel(rows) if nrm else None
    lg = g.logits if form == "logits" else None
    hp, w2 = (None, None) if form == "logits" else (g.hpre, g.W2)
    tail = (rows, d, L, H, SID, key, int(noise))
    tws = (g.tw, g.tb, tc) if tw else (None, None, None)
    if entry == "logits2":
        _call("asrx_abby_fwd_logits2", g.x, lg, g.b2, out, bf16, ys, idx, *tail, *tws)
    elif entry == "logits":
        _call("asrx_abby_fwd_logits", g.x, lg, g.b2, out, ys, idx, *tail)
    elif entry == "fwd2":
        _call("asrx_abby_fwd2", g.x, hp, w2, g.b2, out, bf16, ys, idx, *tail, *tws)
    elif entry == "fwd":
        _call("asrx_abby_fwd", g.x, hp, w2, g.b2, out, ys, idx, *tail)
    elif entry == "fwd3":
        _call("asrx_abby_fwd3", g.x, hp, w2, lg, g.b2, out, bf16, ys, idx, *tail, *tws, nv)
    elif entry == "res":
        _call("asrx_abby_fwd_res", g.x, hp, w2, lg, g.b2, g.res, out, ys, idx, *tail)
    else:
        raise KeyError(entry)
    return types.SimpleNamespace(out=out, ys=ys, idx=idx, nrm=nv, tc=tc)


def _check_fwd(label, got, pair, keep, d, names):
    r64, r32 = pair
    assert bool(torch.isfinite(got.out.float()).all()) and bool(torch.isfinite(got.ys).all()), label
    idx = got.idx.cpu().long()
    assert torch.equal(idx[keep], r64.idx[keep]), (label, (idx != r64.idx).nonzero().flatten()[:8].tolist())
    assert int(idx.min()) >= 0 and int(idx.max()) <= 2, label  # written on every row
    e = {k: v for k, v in A.fwd_errors(got, r64, keep, d).items() if k in names}
    e32 = {k: v for k, v in A.fwd_errors(r32, r64, keep, d).items() if k in names}
    assert set(e) == set(names), (label, set(e), names)
    return A.check(label, e, e32)


def _check_bf16(label, b, f, tc=False):
    assert b.out.dtype == BF16 and torch.equal(b.out, f.out.to(BF16)), label
    assert torch.equal(b.ys, f.ys) and torch.equal(b.idx, f.idx), label
    if tc:
        assert torch.equal(b.tc, f.tc), label


def _modes_and_arms(label, r64, keep):
    assert set(r64.idx[keep].tolist()) == {0, 1, 2}, label
    cond = r64.cond[keep & (r64.idx == 1)]
    assert bool(cond.any()) and not bool(cond.all()), label


OUT = ("out", "edge", "ys")


def _forward_mixed(d, rows, full):
    """Every forward entry point on the mixed tier of one (d, rows); full: the d >= 128 extras and the wrappers."""
    t = A.data("mixed", d, rows)
    tag = f"fwd d={d} r={rows}"
    for form, entry, plain in (("logits", "logits2", "logits"), ("hpre", "fwd2", "fwd")):
        pair = A.fwd_pair(t, form, tw=t.tw, tb=t.tb)
        keep = A.keep_fwd(pair[0], form)
        assert float((~keep).float().mean()) <= A.CAP, (tag, form)
        f = _fwd(entry, t, form)
        _check_fwd(f"{tag} {entry}", f, pair, keep, d, OUT)
        _check_bf16(f"{tag} {entry} bf16", _fwd(entry, t, form, bf16=1), f)
        if rows >= 74:
            _modes_and_arms(f"{tag} {form}", pair[0], keep)
        if not full:
            continue
        w = _fwd(plain, t, form)  # the fp32 wrappers are the same launch
        assert torch.equal(w.out, f.out) and torch.equal(w.ys, f.ys) and torch.equal(w.idx, f.idx), (tag, plain)
        if d < 128:
            continue
        n = _fwd("fwd3", t, form, nrm=True)
        _check_fwd(f"{tag} fwd3-{form}", n, pair, keep, d, OUT + ("nrm",))
        assert torch.equal(n.out, f.out)  # the norm output changes nothing else
        _check_bf16(f"{tag} fwd3-{form} bf16", _fwd("fwd3", t, form, nrm=True, bf16=1), n)
        c = _fwd(entry, t, form, tw=True)
        _check_fwd(f"{tag} {entry}-tc", c, pair, keep, d, OUT + ("tc",))
        _check_bf16(f"{tag} {entry}-tc bf16", _fwd(entry, t, form, tw=True, bf16=1), c, tc=True)
        rp = A.fwd_pair(t, form, res=t.res)
        _check_fwd(f"{tag} res-{form}", _fwd("res", t, form), rp, keep, d, OUT)


@pytest.mark.parametrize("rows", A.SMALL_ROWS)
@pytest.mark.parametrize("d", A.DS)
def test_forward(cuda, d, rows):
    _forward_mixed(d, rows, full=True)


@pytest.mark.parametrize("rows", A.SMALL_ROWS)
@pytest.mark.parametrize("d", A.DS)
def test_forward_ties(cuda, d, rows):
    """Mode 2 on every row, tied window maxima, exact window sums; nothing is left out."""
    t = A.data("ties", d, rows)
    pair = A.fwd_pair(t, "logits")
    assert float(pair[0].cmargin.min()) >= 1e-5 and bool((pair[0].idx == 1).all())
    keep = A.keep_fwd(pair[0], "logits", "ties")
    f = _fwd("logits2", t, "logits")
    _check_fwd(f"fwd-ties d={d} r={rows} logits2", f, pair, keep, d, OUT)
    _check_bf16(f"fwd-ties d={d} r={rows} bf16", _fwd("logits2", t, "logits", bf16=1), f)
    cond = pair[0].cond
    assert rows < 74 or (bool(cond.any()) and not bool(cond.all()))


@pytest.mark.parametrize("d,rows", A.FWD_WRAP, ids=[_id(c) for c in A.FWD_WRAP])
def test_forward_wraps(cuda, d, rows):
    """Past one sweep of the largest grid: both register sets, the break between the arms, the clamped re-read
    of the last row, the LDS rows reused from row to row."""
    _forward_mixed(d, rows, full=False)
    t = A.data("mixed", d, rows)
    pair = A.fwd_pair(t, "hpre")
    n = _fwd("fwd3", t, "hpre", nrm=True)
    _check_fwd(f"fwd d={d} r={rows} fwd3-hpre", n, pair, A.keep_fwd(pair[0], "hpre"), d, OUT + ("nrm",))


NOISE = [(64, 1), (64, 3), (128, 1), (128, 3), (768, 3)]


@pytest.mark.parametrize("d,H", NOISE, ids=[_id(c) for c in NOISE])
def test_forward_noise(cuda, d, H):
    """use_noise = 1: the gumbel draws of oracle.model.Noise.abby on rows (sample, position, head)."""
    from oracle import keys as K
    from oracle import model as om

    B, L = 2, 37
    rows = B * L * H
    seed, step, site = 5, 2, "t.abby"
    t = A.data("mixed", d, rows)
    g = om.Noise(seed, step, torch.float64).abby(site, [SID + b for b in range(B)], H, L)  # (B, H, L, 3)
    g = g.permute(0, 2, 1, 3).reshape(rows, 3).contiguous()
    key = K.site_key(seed, step, site)
    for form, entry in (("hpre", "fwd2"), ("logits", "logits2")):
        pair = A.fwd_pair(t, form, gumbel=g)
        keep = A.keep_fwd(pair[0], "hpre")  # the draws decide the mode on either form: zgap applies to both
        assert float((~keep).float().mean()) <= A.CAP
        got = _fwd(entry, t, form, noise=1, L=L, H=H, key=key)
        _check_fwd(f"fwd-noise d={d} H={H} {entry}", got, pair, keep, d, OUT)
        assert not torch.equal(_fwd(entry, t, form, L=L, H=H, key=key).ys, got.ys)  # the draws were added


# ------------------------------------------------------------------------------------------------ backward
def _backward(tier, d, rows):
    t = A.data(tier, d, rows)
    r64, r32, keep, gy = A.bwd_pair(t)
    assert float((~keep).float().mean()) <= A.CAP
    g = _devs(t)
    gyd, ysd, idxd = dev(gy), dev(r64.ys), r64.idx.to(torch.int32).cuda()
    tag = f"bwd{'-ties' if tier == 'ties' else ''} d={d} r={rows}"
    if rows >= 74:
        cond = r64.cond[keep & (r64.idx == 1)]
        assert bool(cond.any()) and not bool(cond.all())
        assert tier == "ties" or set(r64.idx[keep].tolist()) == {0, 1, 2}
    e32 = A.bwd_errors(r32, r64, keep)
    first = None
    for acc in (0, 1):
        dx = g.old.clone() if acc else sentinel(rows, d)
        dh = sentinel(rows, d)
        dW2, db2 = torch.zeros(3, d, device="cuda"), torch.zeros(3, device="cuda")
        _call("asrx_abby_bwd2", gyd, g.x, g.hpre, g.W2, ysd, idxd, dx, dh, dW2, db2, rows, d, acc)
        got = types.SimpleNamespace(dx=dx, dhpre=dh, dW2=dW2, db2=db2)
        for v in (dx, dh, dW2, db2):
            assert bool(torch.isfinite(v).all()), (tag, acc)
        e = A.bwd_errors(got, r64, keep, old=t.old if acc else None)
        e32a = dict(e32)
        if acc:
            e32a["dx"] = A.row_err(r32.dx + t.old.float(), r64.dx + t.old, keep)
        A.check(f"{tag} acc={acc}", e, e32a)
        first = first or (dx, dh)
    if rows == 74:  # the wrapper is the acc = 0 launch (dx and dhpre are per-row, so equal bit for bit)
        dx2, dh2 = sentinel(rows, d), sentinel(rows, d)
        dW2b, db2b = torch.zeros(3, d, device="cuda"), torch.zeros(3, device="cuda")
        _call("asrx_abby_bwd", gyd, g.x, g.hpre, g.W2, ysd, idxd, dx2, dh2, dW2b, db2b, rows, d)
        assert torch.equal(dx2, first[0]) and torch.equal(dh2, first[1]), tag


@pytest.mark.parametrize("rows", A.SMALL_ROWS)
@pytest.mark.parametrize("d", A.DS)
@pytest.mark.parametrize("tier", ("mixed", "ties"))
def test_backward(cuda, tier, d, rows):
    _backward(tier, d, rows)


# both tiers: in the mixed tier a few rows of large scale carry dW2 / db2, in the ties tier every row weighs the same,
# so a row dropped from a wave's running sums shows whichever rows share that wave
BWD_WRAP = [(tier, d, r) for tier in ("mixed", "ties") for d, r in A.BWD_WRAP]


@pytest.mark.parametrize("tier,d,rows", BWD_WRAP, ids=[_id(c) for c in BWD_WRAP])
def test_backward_wraps(cuda, tier, d, rows):
    """Past one sweep of the 1024-workgroup grid: dW2 / db2 accumulated per wave over several rows, the acc add
    into an old dx, both prefetch depths (AHEAD == 1 at d = 768 and 1024), four rows per wave at d = 64."""
    _backward(tier, d, rows)
