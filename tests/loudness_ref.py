"""numpy restatement of the K-weighted gated loudness (include/diffusynth_hip.h, "loudness"): the coefficients from the stated
formulas, the two biquads as ONE sequential recursion in Python floats (float64), math.fsum for every sum and mean.  Nothing here shares
code with the package.

The keyword defect models are what a kernel can get wrong; tests/test_loudness_cpu.py asserts that each of them moves the integrated loudness
of the gating fixture by more than 1e-3 LU, i.e. that the fixtures can see these faults:
  no_carry                    every chunk of `chunk` samples starts from zero state
  carry_first_stage_only      the shelf's state is carried over a chunk boundary, the high-pass's is dropped
  partial_last_block_counted  a last block that only partly lies inside the signal (zeros behind it) is counted
  gate_in_db_rounded          the gates compare loudnesses rounded to 0.1 dB, not energies"""
import math

import numpy as np

F32 = np.float32
Z_ABS = 10.0 ** ((-70.0 + 0.691) / 10.0)
TABLE_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, -1.99004745483398, 0.99007225036621)


def hop(fs):
    return (fs + 5) // 10


def kweighting(fs):
    """((b, a), (b, a)): shelf, high-pass."""
    f0, g, q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k = math.tan(math.pi * f0 / fs)
    vh = 10.0 ** (g / 20.0)
    vb = vh ** 0.4996667741545416
    a0 = 1.0 + k / q + k * k
    s1 = ([(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0], [1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0])
    f0, q = 38.13547087602444, 0.5003270373238773
    k = math.tan(math.pi * f0 / fs)
    d = 1.0 + k / q + k * k
    s2 = ([1.0, -2.0, 1.0], [1.0, 2.0 * (k * k - 1.0) / d, (1.0 - k / q + k * k) / d])
    return s1, s2


def kfilter(x, fs, *, chunk=256, no_carry=False, carry_first_stage_only=False):
    """y: x through the shelf, then the high-pass, from zero state, sample by sample (transposed direct form II, as scipy.signal.lfilter)."""
    (b1, a1), (b2, a2) = kweighting(fs)
    b10, b11, b12, a11, a12 = b1[0], b1[1], b1[2], a1[1], a1[2]
    b20, b21, b22, a21, a22 = b2[0], b2[1], b2[2], a2[1], a2[2]
    xs = np.asarray(x, F32).astype(np.float64).tolist()
    out = [0.0] * len(xs)
    s0 = s1 = s2 = s3 = 0.0
    broken = no_carry or carry_first_stage_only
    for n, v in enumerate(xs):
        if broken and n % chunk == 0:
            s2 = s3 = 0.0
            if no_carry:
                s0 = s1 = 0.0
        y1 = b10 * v + s0
        s0 = (b11 * v - a11 * y1) + s1
        s1 = b12 * v - a12 * y1
        y2 = b20 * y1 + s2
        s2 = (b21 * y1 - a21 * y2) + s3
        s3 = b22 * y1 - a22 * y2
        out[n] = y2
    return np.array(out, np.float64)


def lufs(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0.0 else -math.inf


def mean(v):
    return math.fsum(v) / len(v) if len(v) else 0.0


def loudness(x, fs, *, chunk=256, no_carry=False, carry_first_stage_only=False, partial_last_block_counted=False, gate_in_db_rounded=False):
    """The definition for one signal -> dict: z (block energies), nb, n1 = |J1|, n2 = |J2|, z_rel, Z, L, threshold, momentary_max."""
    x = np.asarray(x, F32)
    h, n = hop(fs), len(x)
    y2 = kfilter(x, fs, chunk=chunk, no_carry=no_carry, carry_first_stage_only=carry_first_stage_only) ** 2
    nb = max(0, n // h - 3)
    if partial_last_block_counted:
        nb = max(0, -(-n // h) - 3)
        y2 = np.concatenate([y2, np.zeros(4 * h)])
    z = np.array([math.fsum(y2[j * h:(j + 4) * h].tolist()) / (4.0 * h) for j in range(nb)], np.float64)
    if gate_in_db_rounded:
        l = [round(lufs(v), 1) for v in z]
        j1 = [j for j in range(nb) if l[j] > -70.0]
        z_rel = 0.1 * mean([z[j] for j in j1])
        thr = round(lufs(z_rel), 1)
        j2 = [j for j in j1 if l[j] > thr]
    else:
        j1 = [j for j in range(nb) if z[j] > Z_ABS]
        z_rel = 0.1 * mean([z[j] for j in j1])
        j2 = [j for j in j1 if z[j] > z_rel]
    Z = mean([z[j] for j in j2])
    return dict(z=z, nb=nb, n1=len(j1), n2=len(j2), z_rel=z_rel, Z=Z, L=lufs(Z), threshold=lufs(z_rel), momentary_max=max([lufs(v) for v in z], default=-math.inf))


def gain(Z, target_lufs, max_gain):
    """gL of the definition, fp32."""
    if not Z > 0.0:
        return F32(1.0)
    zt = 10.0 ** ((target_lufs + 0.691) / 10.0)
    return F32(min(math.sqrt(zt / Z), float(F32(max_gain))))


# ---------------------------------------------------------------------------------------------------- the test signals
def sine(fs, seconds, freq=997.0, amp=1.0):
    t = np.arange(int(round(fs * seconds)))
    return (amp * np.sin(2.0 * np.pi * freq * t / fs)).astype(F32)


# (seconds, level in dB) of the gating fixture: full level, about -15 dB (chosen so that its ten blocks lie 0.03 to 0.12 dB ABOVE the
# relative threshold: they pass the gate in the energy domain, and nine of them fail one that compares loudnesses rounded to 0.1 dB),
# about -80 dB, -13 dB, and a loud end that stops inside a hop
STRETCHES = ((1.0, 0.0), (1.3, -14.46), (1.0, -80.0), (0.9, -13.0), (0.85, -1.0))


def gating_fixture(fs=16000, seed=0, scale=0.5):
    """A 997 Hz tone, a 40 Hz component of half its amplitude and a little noise, all following the stretches' levels, on a constant DC offset
    of 0.1 (which the level does not scale: the high-pass holds it in its state at every chunk boundary); it ends 837 samples into a hop."""
    rng = np.random.default_rng(seed)
    parts = []
    for sec, db in STRETCHES:
        m = int(round(sec * fs))
        parts.append(np.full(m, 10.0 ** (db / 20.0)))
    lvl = np.concatenate(parts + [np.full(37, 10.0 ** (STRETCHES[-1][1] / 20.0))])
    t = np.arange(len(lvl))
    x = scale * lvl * (np.sin(2 * np.pi * 997.0 * t / fs) + 0.5 * np.sin(2 * np.pi * 40.0 * t / fs) + 0.02 * rng.standard_normal(len(lvl))) + 0.1
    return x.astype(F32)


def noise(n, seed, amp=0.2, dc=0.05, fs=16000):
    """Noise and a 40 Hz component at full level, 0.15 of it and 1e-4 of it (below the absolute gate) by thirds, on a constant DC offset: the
    device tests' signal of any length."""
    rng = np.random.default_rng(7000 + 31 * seed + n)
    t = np.arange(n)
    lvl = np.ones(n)
    third = max(n // 3, 1)
    lvl[third:third + third // 2] = 0.15
    lvl[third + third // 2:2 * third] = 1e-4
    x = lvl * (amp * rng.standard_normal(n) + 0.5 * amp * np.sin(2 * np.pi * 40.0 * t / fs)) + dc
    return x.astype(F32)
