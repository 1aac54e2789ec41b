"""CPU checks of the seeded residual's operand layouts (``engine.seed_pack_host`` / ``engine.seed_panel_index``, the host restatements
the GPU tests compare the kernels' outputs with): the seed K-step emulated lane by lane in the operand layout of
v_mfma_f32_16x16x4_f32, in float32, against float64."""
import numpy as np


def _mfma_16x16x4_f32(a, b, acc):
    """Operand layout of v_mfma_f32_16x16x4_f32: lane 16 k + i of A holds A[row i][k], of B holds B[k][col i]; D[row][col] accumulates
    the four products in float32.  a, b: (64,) float32, acc (16, 16) float32."""
    A, B = a.reshape(4, 16), b.reshape(4, 16)
    for k in range(4):
        acc = (acc + np.outer(A[k], B[k]).astype(np.float32)).astype(np.float32)
    return acc


def test_seed_k_step_layout_and_precision():
    from cmf_amd import engine as E
    rng = np.random.default_rng(3)
    H, W = 4, 14
    w0 = (rng.standard_normal((64, 1, 3, 3)) / 3).astype(np.float32)
    pack = E.seed_pack_host(w0)
    assert pack.shape == (4, 64, 4) and pack.dtype == np.float32 and pack.nbytes == 4096
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    worst = 0.0
    for parity in (0, 1):
        mask = ((ii + jj) % 2 == parity).reshape(-1)
        v = rng.standard_normal((H * W, 16)).astype(np.float32)         # one 16-column slice
        v[~mask] = np.nan                                               # masked pixels may hold anything
        idx = E.seed_panel_index(H, W)
        assert idx.shape == (E.seed_plane(H, W),) and idx.shape[0] >= (H + 2) * (W + 2) + 1
        ok = idx >= 0
        src = np.where(ok, idx, 0)
        panel = np.where((ok & mask[src])[None, :], v[src].T, 0.0).astype(np.float32)   # (16 columns, plane)
        assert np.isfinite(panel).all()
        # float64 reference: conv0 with zero padding on mask . v
        pad = np.zeros((H + 2, W + 2, 16))
        pad[1:-1, 1:-1] = np.where(mask[:, None], v, 0.0).astype(np.float64).reshape(H, W, 16)
        for y in range(H):
            for x in range(W):
                taps = [(dy, dx) for dy in range(3) for dx in range(3)]
                want = sum(w0[:, 0, dy, dx].astype(np.float64)[None, :] * pad[y + dy, x + dx][:, None] for dy, dx in taps)
                want_abs = sum(np.abs(w0[:, 0, dy, dx].astype(np.float64))[None, :] * np.abs(pad[y + dy, x + dx])[:, None] for dy, dx in taps)
                # the kernel's loads: lane (kq, cl) reads 4 floats at plane offset (y + kq)(W + 2) + x of column cl (kq < 3, else zeros) and
                # feeds element j to MFMA j
                a = np.zeros((64, 4), dtype=np.float32)
                for kq in range(3):
                    o = (y + kq) * (W + 2) + x
                    a[16 * kq:16 * kq + 16] = panel[:, o:o + 4]
                got = np.zeros((16, 64), dtype=np.float32)
                for cot in range(4):
                    acc = np.zeros((16, 16), dtype=np.float32)
                    for j in range(3):
                        acc = _mfma_16x16x4_f32(a[:, j], pack[cot, :, j], acc)
                    got[:, 16 * cot:16 * cot + 16] = acc
                # a float32 sum of n = 12 products (three zero ones included): forward bound n 2^-24 sum |w v|
                worst = max(worst, float((np.abs(got - want) / np.maximum(12 * 2.0 ** -24 * want_abs, 1e-300)).max()))
    print(f"seed K-step emulation: worst error / (12 * 2^-24 sum |w v|) = {worst:.3f}")
    assert worst <= 1.0
