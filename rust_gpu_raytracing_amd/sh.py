"""Second-order real spherical harmonics for the probe queries (``Renderer.probe_sh``).

``Renderer.probe_sh`` returns, per probe, the nine sums over its samples of L * b_k(dir) (the
probe contract in include/rt_abi.h) with directions uniform on the sphere. The functions here
turn those sums into radiance along a direction and into irradiance for a normal. Pure NumPy,
float64 throughout; the order of the coefficients and their signs are the contract's:

    b0 = 1/2 sqrt(1/pi)
    b1 = 1/2 sqrt(3/pi) y          b2 = 1/2 sqrt(3/pi) z          b3 = 1/2 sqrt(3/pi) x
    b4 = 1/2 sqrt(15/pi) x y       b5 = 1/2 sqrt(15/pi) y z
    b6 = 1/4 sqrt(5/pi) (3 z^2 - 1)
    b7 = 1/2 sqrt(15/pi) x z       b8 = 1/4 sqrt(15/pi) (x^2 - y^2)

(the contract's f32 literals are these constants rounded to eight digits).
"""
import numpy as np

_C0 = 0.5 * np.sqrt(1.0 / np.pi)
_C1 = 0.5 * np.sqrt(3.0 / np.pi)
_C2 = 0.5 * np.sqrt(15.0 / np.pi)
_C20 = 0.25 * np.sqrt(5.0 / np.pi)
_C22 = 0.25 * np.sqrt(15.0 / np.pi)

# The cosine lobe's zonal coefficients per band (Ramamoorthi and Hanrahan 2001): A_0, A_1, A_2,
# spread over the nine coefficients.
BAND = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])
COSINE_LOBE = np.array([np.pi, 2.0 * np.pi / 3.0, np.pi / 4.0])[BAND]


def basis(dirs):
    """The nine basis values of each direction: ``dirs`` (..., 3), assumed of unit length, gives
    (..., 9) float64."""
    d = np.asarray(dirs, np.float64)
    if d.shape[-1:] != (3,):
        raise ValueError("dirs must have shape (..., 3)")
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, _C0), _C1 * y, _C1 * z, _C1 * x, _C2 * (x * y), _C2 * (y * z),
                     _C20 * (3.0 * (z * z) - 1.0), _C2 * (x * z), _C22 * (x * x - y * y)], axis=-1)


def _coefficients(sh, samples):
    sh = np.asarray(sh, np.float64)
    if sh.ndim < 2 or sh.shape[-2] != 9:
        raise ValueError("sh must have shape (..., 9, channels)")
    if samples <= 0:
        raise ValueError("samples must be positive")
    return sh * (4.0 * np.pi / samples)


def radiance(sh, dirs, samples):
    """The band-limited radiance arriving from ``dirs``: sum_k sh_k b_k(dir) * 4 pi / samples.
    ``sh`` (..., 9, c) as ``Renderer.probe_sh`` returns it for ``samples`` samples, ``dirs``
    (..., 3) broadcast against it; returns (..., c) float64."""
    return np.einsum("...kc,...k->...c", _coefficients(sh, samples), basis(dirs))


def irradiance(sh, normals, samples):
    """The irradiance of a surface with unit normal ``normals`` at the probe: the radiance
    convolved with the clamped cosine lobe, A_0 = pi, A_1 = 2 pi / 3, A_2 = pi / 4 per band.
    Shapes as in ``radiance``. Divide by pi for the radiance a white diffuse surface reflects."""
    return np.einsum("...kc,...k->...c", _coefficients(sh, samples), basis(normals) * COSINE_LOBE)
