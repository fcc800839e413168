"""Layout FID: the Fréchet distance between LayoutNet feature statistics of the dataset's layouts and of the generator's
(reference: metrics/layout_frechet_inception_distance.py:20-39; "GANs trained by a two time-scale update rule ...", Heusel et al.)."""
import numpy as np

from . import metric_utils_layout

#----------------------------------------------------------------------------

def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr(sigma1) + tr(sigma2) - 2 tr sqrt(sigma1 sigma2), float64 on the host.  tr sqrt(A) is the sum of the square roots of A's
    eigenvalues (numpy.linalg.eigvals; real parts, as the reference keeps the real part of scipy.linalg.sqrtm's result, :37-38): the eigenvalues
    of a product of two covariance matrices are real and >= 0 up to rounding, where the principal root is taken as well."""
    mu1, mu2 = np.asarray(mu1, dtype=np.float64), np.asarray(mu2, dtype=np.float64)
    sigma1, sigma2 = np.asarray(sigma1, dtype=np.float64), np.asarray(sigma2, dtype=np.float64)
    m = np.square(mu1 - mu2).sum()
    lam = np.linalg.eigvals(np.dot(sigma1, sigma2))
    tr_sqrt = np.sqrt(lam.astype(np.complex128)).real.sum()
    return float(m + np.trace(sigma1) + np.trace(sigma2) - 2.0 * tr_sqrt)

#----------------------------------------------------------------------------

def compute_layout_fid(opts, max_real, num_gen):
    dataset_name = opts.dataset_kwargs['path'].split('/')[-3]
    detector_pth = 'pretrained/layoutnet_%s.pth.tar' % dataset_name
    detector_kwargs = dict(return_features=True) # Return raw features before the softmax layer.

    mu_real, sigma_real = metric_utils_layout.compute_feature_stats_for_dataset(
        opts=opts, detector_pth=detector_pth, detector_kwargs=detector_kwargs,
        rel_lo=0, rel_hi=0, capture_mean_cov=True, max_items=max_real).get_mean_cov()

    mu_gen, sigma_gen = metric_utils_layout.compute_feature_stats_for_generator(
        opts=opts, detector_pth=detector_pth, detector_kwargs=detector_kwargs,
        rel_lo=0, rel_hi=1, capture_mean_cov=True, max_items=num_gen).get_mean_cov()

    if opts.rank != 0:
        return float('nan')
    return frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real)

#----------------------------------------------------------------------------
