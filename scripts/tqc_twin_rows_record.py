"""Records what the twin critic loss kernel of the commit before the fold wrote — truncated_quantile_critic_loss_kernel
through tonic_debug_truncated_quantile_loss, an entry this commit no longer has — on the crafted rows of
tests/test_gpu_tqc.py (LOSS_CASES x LOSS_BATCHES), as the fixture tests/golden/tqc_twin_loss_parent.npz that
test_loss_kernel_equals_the_retired_twin_kernel compares the kept kernel with:

    python scripts/tqc_twin_rows_record.py --tree <a built checkout of that commit> --out tests/golden/tqc_twin_loss_parent.npz

Per case M<M>_d<d>_B<B>: _dlogits_1, _dlogits_2 [B, ld], _sample_m [3, B] and _inputs_sha256 of the rows (this
checkout's crafted_rows: the rows are made here, the kernel runs there).  Outputs only, compressed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--tree', required=True)
    parser.add_argument('--out', required=True)
    args = parser.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]      # (as tests/conftest.py)
    import numpy as np
    import torch
    import tonic_amd
    from tonic_amd import _lib
    import test_gpu_tqc as cases
    assert os.path.abspath(tonic_amd.__file__).startswith(tree), tonic_amd.__file__
    assert torch.cuda.is_available(), 'the kernel runs on the GPU'
    lib, p, out = _lib.load(), _lib.ptr, {}
    for M, d in cases.LOSS_CASES:
        for B in cases.LOSS_BATCHES:
            rows, _ = cases.crafted_rows(B, M)
            ld, Bp = cases.pad16(M), cases.pad16(B)

            def padded(x, fill):
                full = torch.full((B, ld), fill, dtype=torch.float32)
                full[:, :M] = x
                return full.cuda()
            t1, t2 = padded(rows['target_1'], 777.0), padded(rows['target_2'], -777.0)
            th1, th2 = padded(rows['theta_1'], float('nan')), padded(rows['theta_2'], 555.0)
            r, disc, logp = rows['rewards'].cuda(), rows['discounts'].cuda(), rows['logp'].cuda()
            g1, g2 = (torch.full((B, ld), float('nan'), device='cuda') for _ in range(2))
            sample_m = torch.full((3, Bp), float('nan'), device='cuda')
            _lib.check(lib.tonic_debug_truncated_quantile_loss(
                p(t1), p(t2), p(th1), p(th2), ld, p(r), p(disc), p(logp), M, d, cases.ALPHA, None, p(g1), p(g2),
                p(sample_m), B, Bp, _lib.current_stream()), 'tonic_debug_truncated_quantile_loss')
            torch.cuda.synchronize()
            key = f'M{M}_d{d}_B{B}'
            out[key + '_dlogits_1'], out[key + '_dlogits_2'] = g1.cpu().numpy(), g2.cpu().numpy()
            out[key + '_sample_m'] = sample_m[:, :B].cpu().numpy()
            out[key + '_inputs_sha256'] = np.array(cases.rows_digest(rows))
            assert np.isfinite(out[key + '_sample_m']).all() and np.isfinite(out[key + '_dlogits_1']).all()
    np.savez_compressed(args.out, **out)
    print(f'{len(out) // 4} cases -> {args.out}')


if __name__ == '__main__':
    main()
