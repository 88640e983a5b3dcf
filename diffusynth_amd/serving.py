"""Mixed-width note batches: the MIDI arranger and the text2sound tab ask for notes of different
durations, i.e. latents of different widths (webUI/natural_language_guided_4/track_maker.py:245, text2sound.py:84:
``width = int(256 * ((duration + 1) / 4) / 4)``, any integer in [20, 144]).

The reference serves them one ``sample()`` call per note.  Here one call takes the whole request list: every request is a
batch-1 ``sample()`` call submitted to a SamplingBatcher (batching.py), one width at a time, so the requests of equal width are
one U-Net batch (one plan of the engine, which keeps all plans in one bounded arena — engine.py:_cached_plan) stepped together;
the results come back in request order.
No padding to a common width is involved: a note's convolution borders, GroupNorm counts and attention length are those
of its own width, so each request's result is what its own single-sample call would have produced (bit for bit in the
fp32 tier — and in the bf16x3 / bf16 tiers on a model pinned with ``model.pin_launch_batch(n)`` — with the deterministic samplers,
"ddim" and "dpmpp_2m", where a request's result does not depend on per-step noise)."""
import numpy as np
import torch

from .sampler import DiffSynthSampler, mix_weights


def _request_mix(r, unconditional_condition):
    """The weights of a multi-prompt request as float32 numpy, (K,) or (K, width) — None for a single-prompt request."""
    if "conditions" not in r and "weights" not in r:
        return None
    if r.get("condition") is not None:
        raise ValueError("a request carries either 'condition' or 'conditions' with 'weights', not both")
    if r.get("conditions") is None or r.get("weights") is None:
        raise ValueError("a multi-prompt request needs both 'conditions' (K, D) and 'weights' (K,) or (K, width)")
    if unconditional_condition is None:
        raise ValueError("a multi-prompt request needs an unconditional_condition (the negative-prompt embedding)")
    w = mix_weights(r["weights"])                   # (K in 1 ... 8, finite values: the sampler's own checks)
    K, width = r["conditions"].shape[0], int(r["width"])
    if r["conditions"].dim() != 2 or w.shape not in ((K,), (K, width)):
        raise ValueError("weights must be (K,) or (K, width) = (%d,) or (%d, %d) for conditions (K, D), got weights %r and conditions %r"
                         % (K, K, width, tuple(w.shape), tuple(r["conditions"].shape)))
    return w


@torch.no_grad()
def sample_mixed_widths(model, requests, steps, *, timesteps=1000, height=128, channels=4, sampler="ddim", cfg_scale=1.0,
                        unconditional_condition=None, device="cuda", noise_device=None, return_trajectory=False, use_timesteps=None,
                        guidance_rescale=0.0):
    """requests: list of dicts ``{"width": int, "condition": (label_dim,) tensor or None, "seed": int}``.
    Returns a list (request order) of final latents (4, height, width) — or of trajectories when asked.
    Instead of ``"condition"`` a request may carry ``"conditions": (K, label_dim)`` with ``"weights": (K,)`` or ``(K, width)``: K prompts
    guiding one sound (``DiffSynthSampler.set_condition_mix``; needs ``unconditional_condition``, ``cfg_scale == 1`` is allowed).  Such
    a request takes 1 + K U-Net rows.  Both forms in one request, or weights that do not match K and the width, raise ``ValueError``.

    Each request's initial noise is drawn like a batch-1 reference call with its seed would draw it
    (``torch.manual_seed(seed)``; ``randn((1, C, H, train_width))``, on a private generator); requests of one width then share the
    loop.  ``use_timesteps`` (a list for ``DiffSynthSampler.respace``, e.g. ``logsnr_timesteps(steps)``) replaces the default
    ``linspace(0, timesteps - 1, steps)``.  ``guidance_rescale`` is every sampler's
    ``activate_classifier_free_guidance(..., guidance_rescale=)`` (stored, not applied, with ``cfg_scale == 1``).

    Only the deterministic samplers ("ddim", "dpmpp_2m") are served this way: with ``"ddpm"`` the per-step noise of a bucket would come from ONE
    generator stream, so a request's result would depend on which other requests share its width and on their order (the
    reference serves one call per note, so that case has no reference behaviour to match)."""
    if sampler not in ("ddim", "dpmpp_2m"):
        raise NotImplementedError("sample_mixed_widths serves the deterministic samplers ('ddim', 'dpmpp_2m') only: per-step noise of a "
                                  "shared bucket would make a request's result depend on its bucket mates (got %r)" % (sampler,))
    if cfg_scale != 1.0 and unconditional_condition is None:
        raise ValueError("cfg_scale != 1 needs an unconditional_condition (the negative-prompt embedding)")
    mixes = [_request_mix(r, unconditional_condition) for r in requests]        # (every request is checked before any device work)
    from .batching import SamplingBatcher
    # one group per (width, condition present), run one after the other: every group is one U-Net batch (as many plans are built as
    # there are groups, however many widths the list holds — the engine keeps DS_MAX_PLANS), and every request a batch-1 call
    groups = {}
    for i, r in enumerate(requests):
        groups.setdefault((int(r["width"]), r.get("condition") is None and mixes[i] is None), []).append(i)
    # U-Net rows of a request: 1 + K with a mix of K prompts, 2 under CFG, 1 otherwise
    # (times the windows of its width on a windowed model, diffusynth_amd.windowed)
    rps = getattr(model, "rows_per_sample", lambda width: 1)
    need = [((2 if cfg_scale != 1.0 else 1) if m is None else 1 + m.shape[0]) * int(rps(int(r["width"]))) for m, r in zip(mixes, requests)]
    rows = max(sum(need[i] for i in idxs) for idxs in groups.values()) if groups else 1
    b = SamplingBatcher(model, max_rows=rows)
    out = [None] * len(requests)
    for (width, nocond), idxs in groups.items():
        handles = []
        for i in idxs:
            s = DiffSynthSampler(timesteps, mute=True, device=device, height=height, max_batchsize=1, channels=channels,
                                 noise_device=noise_device)
            s.respace(list(np.linspace(0, timesteps - 1, steps, dtype=np.int32)) if use_timesteps is None else list(use_timesteps))
            if cfg_scale != 1.0 or guidance_rescale != 0.0 or mixes[i] is not None:
                s.activate_classifier_free_guidance(cfg_scale, unconditional_condition, guidance_rescale)
            if mixes[i] is not None:
                s.set_condition_mix(mixes[i])
                c = requests[i]["conditions"].to(device).float()[None]
            else:
                c = None if nocond else requests[i]["condition"].to(device).float()[None]
            handles.append(b.submit(s, "sample", (1, channels, height, width), return_tensor=True, condition=c, sampler=sampler,
                                    seed=int(requests[i]["seed"])))
        b.run()
        for i, h in zip(idxs, handles):
            imgs, _ = h.result()
            out[i] = [im[0] for im in imgs] if return_trajectory else imgs[-1][0]
    return out


@torch.no_grad()
def inpaint_with_text(model, requests, steps, *, timesteps=1000, height=128, channels=4, sampler="ddim", cfg_scale=1.0,
                      unconditional_condition=None, device="cuda", noise_device=None, noise_strategy="repeat", train_width=64,
                      max_width=256, VAE_scale=4, time_resolution=256, guidance_rescale=0.0):
    """The Inpaint tab for a list of requests (webUI/natural_language_guided_4/inpaint_with_text.py:193-267): each request's drawing
    becomes its latent mask on the device (diffusynth_amd.inpaint_mask: all masks of the list in one pass of the three kernels) and its
    ``inpaint_sample`` call is submitted to one SamplingBatcher with the one-channel plane as the mask.  requests: list of dicts

        ``{"guide": (1, channels, height, W) latent (what InputBatch2Encode_STFT returned), "layers": the ImageEditor's layers``
        ``(list of (H, W, 4) uint8) or "mask": the merged 2-D 0/1 array, "time_range": (begin, end) or None, "freq_range": (begin, end)``
        ``or None, "inpaint_area": "masked" / "unmasked" (default), "condition": (label_dim,) tensor, "seed": int,``
        ``"noising_strength": float in (0, 1], "batchsize": int (default 1), "width": int (default: the guide's)}``

    The guide is what the sampler's noise strategy takes as one: ``train_width`` columns under "repeat", which the sampler repeats or
    crops to the call's ``width`` as it does the noise (the arranger's notes: track_maker.py:245-269), ``max_width`` under
    "non_repeat"; both are handed to the samplers built here.  The reference's tab has ``width = guide.shape[-1]`` (:249), the default here; the drawing is ``VAE_scale * width`` wide.

    Returns a list (request order) of final latents ``(batchsize, channels, height, width)``.  A request is the reference's call: the guide
    repeated ``batchsize`` times, the condition likewise, a sampler respaced to ``int(steps / noising_strength)`` steps (:244-246),
    ``inpaint_sample(shape, seed=, noising_strength=, guide_img=, mask=, condition=, sampler=)`` on a ``DiffSynthSampler(timesteps,
    height=, channels=, noise_strategy=)``.  The rules of ``sample_mixed_widths`` hold: the deterministic samplers only, every request is
    checked before any device work (the drawings too: ``ValueError`` as ``latent_mask_from_layers`` raises it), requests of one width
    share their U-Net steps."""
    if sampler not in ("ddim", "dpmpp_2m"):
        raise NotImplementedError("inpaint_with_text serves the deterministic samplers ('ddim', 'dpmpp_2m') only: per-step noise of a "
                                  "shared bucket would make a request's result depend on its bucket mates (got %r)" % (sampler,))
    if cfg_scale != 1.0 and unconditional_condition is None:
        raise ValueError("cfg_scale != 1 needs an unconditional_condition (the negative-prompt embedding)")
    from . import inpaint_mask as M
    from .batching import SamplingBatcher
    requests = list(requests)
    if not requests:
        return []
    guide_width = int(train_width if noise_strategy == "repeat" else max_width)
    shapes, counts = [], []
    for i, r in enumerate(requests):
        if ("layers" in r) == ("mask" in r):
            raise ValueError("request %d carries either 'layers' or 'mask' (got %s)" % (i, "both" if "layers" in r else "neither"))
        g, B = r["guide"], int(r.get("batchsize", 1))
        if g.dim() != 4 or tuple(g.shape) != (1, channels, height, guide_width):
            raise ValueError("request %d: the guide must be (1, %d, %d, %d) for noise_strategy %r, got %r"
                             % (i, channels, height, guide_width, noise_strategy, tuple(g.shape)))
        width = int(r.get("width", g.shape[3]))
        if width < 1:
            raise ValueError("request %d: width must be >= 1 (got %r)" % (i, r.get("width")))
        if B < 1:
            raise ValueError("request %d: batchsize must be >= 1 (got %r)" % (i, r.get("batchsize")))
        ns = float(r["noising_strength"])
        if not 0.0 < ns <= 1.0 or not 1 <= int(steps / ns) <= timesteps:
            raise ValueError("request %d: noising_strength %r with %r steps gives %r sampler steps" % (i, r["noising_strength"], steps, ns and int(steps / ns)))
        c = r.get("condition")
        if c is None and cfg_scale != 1.0:
            raise ValueError("request %d: classifier-free guidance (cfg_scale != 1) needs a condition" % i)
        if c is not None and (not isinstance(c, torch.Tensor) or c.dim() != 1 or not c.is_floating_point()):
            raise ValueError("request %d: the condition must be a (label_dim,) float tensor, got %r"
                             % (i, tuple(c.shape) if isinstance(c, torch.Tensor) else type(c).__name__))
        seed = r.get("seed")
        if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)):
            raise ValueError("request %d: seed must be an int (got %r)" % (i, seed))
        shapes.append((B, channels, height, width))
        counts.append(int(steps / ns))
    specs = M.plan_masks([r["layers"] if "layers" in r else r["mask"] for r in requests], shapes, VAE_scale, time_resolution,
                         [r.get("time_range") for r in requests], [r.get("freq_range") for r in requests],
                         [r.get("inpaint_area", "unmasked") for r in requests])
    planes, _ = M.run_masks(specs, device)
    rps = getattr(model, "rows_per_sample", lambda width: 1)
    need = [s[0] * (2 if cfg_scale != 1.0 else 1) * int(rps(s[3])) for s in shapes]
    b = SamplingBatcher(model, max_rows=max(128, max(need)))      # (the batcher's default, or what the largest request alone takes)
    handles = []
    for r, shape, n, plane in zip(requests, shapes, counts, planes):
        s = DiffSynthSampler(timesteps, mute=True, device=device, height=height, channels=channels, noise_strategy=noise_strategy,
                             train_width=train_width, max_width=max_width, max_batchsize=max(16, shape[0]), noise_device=noise_device)
        s.respace(list(np.linspace(0, timesteps - 1, n, dtype=np.int32)))
        if cfg_scale != 1.0 or guidance_rescale != 0.0:
            s.activate_classifier_free_guidance(cfg_scale, unconditional_condition, guidance_rescale)
        c = None if r.get("condition") is None else r["condition"].to(device).float()[None].repeat(shape[0], 1)
        guide = r["guide"].to(device).float().repeat(shape[0], 1, 1, 1)
        handles.append(b.submit(s, "inpaint_sample", shape, float(r["noising_strength"]), guide, plane, return_tensor=True, condition=c,
                                sampler=sampler, seed=int(r["seed"])))
    b.run()
    return [h.result()[0][-1] for h in handles]
