"""A numpy restatement of the random stream of the device Monte Carlo moves (include/remd_hip_mcmoves.h, csrc/mc_moves.hip):
REMD_STREAM_MC_MOVE = 8, counter a = 4 * position + block, b = global replica, t = iteration.  Blocks 0 and 1 give the four
proposal uniforms, block 2 the acceptance uniform.  The Philox words come from the oracle package's C implementation; every
formula below is written in f64 with numpy's library functions."""
import numpy as np
import oracle

STREAM_MC_MOVE = 8


def u53(hi, lo):
    """53-bit uniform in [0, 1) of two words (csrc/rng.h remd_u53)."""
    return float((int(hi) << 21) | (int(lo) >> 11)) / 9007199254740992.0


def uniforms(seed, iteration, position, replica):
    """u0 .. u3 of the proposal."""
    a = oracle.draw(int(seed), STREAM_MC_MOVE, 4 * int(position), int(replica), int(iteration))
    b = oracle.draw(int(seed), STREAM_MC_MOVE, 4 * int(position) + 1, int(replica), int(iteration))
    return u53(a[0], a[1]), u53(a[2], a[3]), u53(b[0], b[1]), u53(b[2], b[3])


def acceptance_uniform(seed, iteration, position, replica):
    w = oracle.draw(int(seed), STREAM_MC_MOVE, 4 * int(position) + 2, int(replica), int(iteration))
    return u53(w[2], w[3])


def normals(seed, iteration, position, replica):
    """The three standard normals of a displacement (Box-Muller; the vector is sigma times these)."""
    u0, u1, u2, u3 = uniforms(seed, iteration, position, replica)
    rxy, rz = np.sqrt(-2.0 * np.log(1.0 - u0)), np.sqrt(-2.0 * np.log(1.0 - u2))
    return np.array([rxy * np.cos(2.0 * np.pi * u1), rxy * np.sin(2.0 * np.pi * u1), rz * np.cos(2.0 * np.pi * u3)])


def displacement(seed, iteration, position, replica, sigma_nm):
    return float(sigma_nm) * normals(seed, iteration, position, replica)


def quaternion(seed, iteration, position, replica):
    """Shoemake's uniform quaternion, the reference's formula (mcmc.py:1882-1906), of u0, u1, u2."""
    u0, u1, u2, _ = uniforms(seed, iteration, position, replica)
    return np.array([np.sqrt(1.0 - u0) * np.sin(2.0 * np.pi * u1), np.sqrt(1.0 - u0) * np.cos(2.0 * np.pi * u1),
                     np.sqrt(u0) * np.sin(2.0 * np.pi * u2), np.sqrt(u0) * np.cos(2.0 * np.pi * u2)])


def rotation_matrix(seed, iteration, position, replica):
    """The reference's matrix of that quaternion (mcmc.py:1842-1880), written out here on its own."""
    w, x, y, z = quaternion(seed, iteration, position, replica)
    s = 2.0 / (w * w + x * x + y * y + z * z)
    return np.array([[1.0 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
                     [s * (x * y + w * z), 1.0 - s * (x * x + z * z), s * (y * z - w * x)],
                     [s * (x * z - w * y), s * (y * z + w * x), 1.0 - s * (x * x + y * y)]])


def displace(x, seed, iteration, position, replica, sigma_nm):
    """f64 result of the displacement of the f32 positions x [n][3]."""
    return np.asarray(x, dtype=np.float64) + displacement(seed, iteration, position, replica, sigma_nm)


def rotate(x, seed, iteration, position, replica):
    """f64 result of the rotation of the f32 positions x [n][3] about their centre of geometry."""
    x = np.asarray(x, dtype=np.float64)
    centre = x.mean(0)
    return (rotation_matrix(seed, iteration, position, replica) @ (x - centre).T).T + centre


def accepts(delta, u):
    """The decision of csrc/mc_moves.hip: accept when delta <= 0 or u < exp(-delta); a NaN rejects."""
    return bool(delta <= 0.0 or u < np.exp(-delta))
