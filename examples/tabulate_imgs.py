"""Counterpart of the reference's experiments/tabulators/tabulate_imgs.py (Tables 2 and 3; LPIPS left out: its AlexNet
weights are not a dependency) and, with --autocorr, of plot_autocorrs_imgs.py (the curves of Figure 8, printed): PSNR and
SSIM of the result files examples/imgs_restore.py writes, scored on the device by fbs_amd.image_metrics.

    python examples/tabulate_imgs.py --outdir imgs/results --dataset mnist --task supr-4 --nparticles 100 --ny0s 100 \
        --methods filter gibbs-eb-ef pmcmc-0.005 twisted csgm --autocorr --max_lags 20
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbs_amd.image_metrics import tabulate_autocorr, tabulate_images  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser(description='PSNR / SSIM table and autocorrelation curves of restored images.')
    p.add_argument('--outdir', type=str, default='./imgs/results')
    p.add_argument('--dataset', type=str, default='mnist')
    p.add_argument('--task', type=str, default='supr-4', help="As in the file names: 'inpaint-15', 'supr-4'.")
    p.add_argument('--sde', type=str, default='lin')
    p.add_argument('--nparticles', type=int, default=100)
    p.add_argument('--ny0s', type=int, default=100)
    p.add_argument('--methods', type=str, nargs='+', default=['filter', 'gibbs-eb-ef', 'pmcmc-0.005', 'twisted', 'csgm'],
                   help="As on the driver's command line, with '-marg' appended where it ran with --marg.")
    p.add_argument('--autocorr', action='store_true', help='Also the best-variable autocorrelation of the chain methods.')
    p.add_argument('--max_lags', type=int, default=20)
    args = p.parse_args(argv)
    where = (args.outdir, args.dataset, args.task, args.sde, args.nparticles, args.methods, args.ny0s)
    table = tabulate_images(*where)
    for method, row in table.items():
        print(f"{method} | PSNR: {row['psnr'][0]:.4f} {row['psnr'][1]:.4f} | SSIM: {row['ssim'][0]:.4f} {row['ssim'][1]:.4f}")
    curves = tabulate_autocorr(*where, max_lags=args.max_lags) if args.autocorr else {}
    for method, curve in curves.items():
        print(f"{method} | autocorrelation (best variable), lags 0..{len(curve) - 1}: " + ' '.join(f'{v:.4f}' for v in curve))
    return table, curves


if __name__ == '__main__':
    main()
