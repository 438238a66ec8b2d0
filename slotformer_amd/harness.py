"""Counterparts of the reference's offline drivers around the hot path.

The reference scripts mix dataset I/O, nn.DataParallel and pickling with a few lines of index
arithmetic; only that arithmetic and the model calls are reproduced here, operating on tensors.
"""
import torch

from . import engine

OBS_FRAMES = 128   # rollout_clevrer_slots.py:15
TARGET_LEN = 160   # rollout_clevrer_slots.py:16


@torch.no_grad()
def extract_video_slots(model, videos, batch_size=1):
    """H1 -- extract_slots.py:19-38.  videos: [V, T, 3, H, W] (tensor or list of [T,3,H,W]) ->
    float32 numpy-ready tensor [V, T, N, D] on the host.  `model` is a StoSAVi / STEVE in eval
    mode with testing=True; whole videos are encoded, `batch_size` videos per engine call."""
    model.eval()
    assert model.testing, 'set model.testing = True for slot extraction (extract_slots.py:127)'
    key = 'post_slots' if hasattr(model, 'kernel_dist_layer') else 'slots'
    out = []
    n = len(videos)
    for s in range(0, n, batch_size):
        clip = videos[s:s + batch_size]
        if not torch.is_tensor(clip):
            clip = torch.stack(list(clip), 0)
        res = model({'img': clip.float().to(model.device)})
        out.append(res[key].detach().cpu())
    return torch.cat(out, 0)


@torch.no_grad()
def rollout_video_slots(model, ori_slots, frame_offset, history_len=None, obs_frames=OBS_FRAMES,
                        target_len=TARGET_LEN, one_call=False):
    """H2 -- rollout_clevrer_slots.py:20-65 / rollout_physion_slots.py:22-63.

    ori_slots [B, obs_frames, N, C] -> [B, target_len, N, C]: for every offset `off` the strided
    sub-sequence start::frame_offset (start = obs - hist*offset + off) is rolled out for as many
    steps as it has frames beyond the burn-in, and the predictions are interleaved back.

    one_call=False restates the reference: a gathered copy and one model call of B videos per offset, then the interleave.
    one_call=True: the frame_offset phases of every video as ONE engine rollout of B * frame_offset videos that reads and writes the
    frames where they lie (`engine.rollout_phases`) -- one buffer padded to whole steps, sliced to target_len (a view).
    """
    model.eval()
    hist = model.history_len if history_len is None else history_len
    dev = model.device
    ori = ori_slots.float().to(dev)
    B, _, N, C = ori.shape
    if one_call:
        if hist != engine.burn_in_of(model.rollouter):
            raise ValueError(f'slotformer_amd.harness: one_call=True runs the rollouter\'s own burn-in of {engine.burn_in_of(model.rollouter)} frames, '
                             f'got history_len={hist}')
        pred_len = target_len - obs_frames
        steps = -(-pred_len // frame_offset)
        buf = torch.empty(B, obs_frames + steps * frame_offset, N, C, device=dev)
        buf[:, :obs_frames].copy_(ori[:, :obs_frames])
        engine.rollout_phases(model.rollouter, buf, obs_frames, pred_len, frame_offset)
        return buf[:, :target_len]
    full = torch.cat([ori, torch.zeros(B, target_len - obs_frames, N, C, device=dev)], 1)
    preds = []
    for off in range(frame_offset):
        start = obs_frames - hist * frame_offset + off
        in_slots = full[:, start::frame_offset].contiguous()
        model.rollout_len = in_slots.shape[1] - hist
        preds.append(model({'slots': in_slots})['pred_slots'])
    pred = torch.stack([preds[i % frame_offset][:, i // frame_offset] for i in range(target_len - obs_frames)], 1)
    out = torch.cat([full[:, :obs_frames], pred], 1)
    assert out.shape[1] == target_len
    return out


@torch.no_grad()
def extract_video_tokens(dvae, videos, batch_size=64, ingest=None, to_host=True):
    """base_slots/tokenize_images.py:15-40 -- the dVAE token ids of whole clips, as the token files hold them.  videos [N, T, 3, H, W] float
    frames (anything `.float()` takes), on the device or on the host -> int16 [N, T, h*w], in pinned host memory with to_host=True (what
    `slot_io.save_video_tokens` writes), on the device otherwise.  The frames go through `dvae.tokenize_ids` in chunks of `batch_size` FRAMES (a clip
    may span chunks; the last chunk may be shorter): no logits buffer anywhere, and only a chunk of a host-resident set is on the device at a
    time.  Each chunk's ids are written straight into the result; the download of a chunk runs on a side stream behind the next chunk's kernels.
    ingest: an `ingest.FrameIngest` -- `videos` is then the decoder's RAW uint8 clips [N, T, H0, W0, 3] ([N, T, H0, W0] with a palette), normalised
    and resized on the device chunk by chunk, as `extract_and_rollout` takes them."""
    if int(batch_size) < 1:
        raise ValueError(f'slotformer_amd.harness: batch_size >= 1, got {batch_size!r}')
    if dvae.vocab_size > 32768:
        raise ValueError(f'slotformer_amd.harness: int16 token files cannot hold a vocabulary of {dvae.vocab_size}')
    dev = dvae.device
    if ingest is None:
        if videos.dim() != 5:
            raise ValueError(f'slotformer_amd.harness: clips are [N, T, 3, H, W], got {tuple(videos.shape)}')
        N, T, _, H, W = videos.shape
    else:
        shape = ingest.output_shape(videos)   # (raises for anything but contiguous uint8 frames)
        if videos.dim() != (4 if ingest.palette is not None else 5):
            raise ValueError(f'slotformer_amd: ingest= takes clips [N, T, H0, W0, 3] ([N, T, H0, W0] with a palette), got {tuple(videos.shape)}')
        N, T, H, W = shape[0], shape[1], shape[-2], shape[-1]
    flat = videos.reshape((N * T, ) + tuple(videos.shape[2:]))
    hw = (H // 4) * (W // 4)
    F_ = N * T
    out = torch.empty(F_, hw, dtype=torch.int16, pin_memory=True) if to_host else torch.empty(F_, hw, dtype=torch.int16, device=dev)
    copies, keep = (torch.cuda.Stream(device=dev), []) if to_host else (None, None)
    for a, b in render_chunks(F_, batch_size):
        chunk = flat[a:b].to(dev, non_blocking=True)
        chunk = ingest(chunk) if ingest is not None else chunk.float()
        if not to_host:
            dvae.tokenize_ids(chunk, out=out[a:b], dtype=torch.int16)
            continue
        ids = dvae.tokenize_ids(chunk, dtype=torch.int16)
        ready = torch.cuda.Event()
        ready.record()
        copies.wait_event(ready)
        with torch.cuda.stream(copies):
            out[a:b].copy_(ids.view(b - a, hw), non_blocking=True)
        keep.append(ids)   # alive until its copy has run
    if to_host:
        copies.synchronize()
    return out.view(N, T, hw)


def render_chunks(num_frames, frames_per_call=64):
    """[(start, stop), ...] covering range(num_frames) once, `frames_per_call` frames per chunk (the last one may be shorter)."""
    if int(frames_per_call) < 1:
        raise ValueError(f'slotformer_amd.harness: frames_per_call >= 1, got {frames_per_call!r}')
    return [(s, min(s + int(frames_per_call), num_frames)) for s in range(0, num_frames, int(frames_per_call))]


@torch.no_grad()
def render_video_slots(model, slots, frames_per_call=64, soft=False, to_host=False, fused=False, seed=None, sample=False, temperature=1.0,
                       sample_seed=None):
    """The device form of STEVE's `_slots2video` (video_prediction/method.py:207-219): slots [V,T,N,D] or [T,N,D] -> the frames
    `model.render` draws from them (the hard image; with soft=True the Gumbel-softmax one), float32 [V,T,3,H,W] / [T,3,H,W] on the
    device.  `model` is a STEVESlotFormer or STEVE in eval mode.  The frames go through `render` in chunks of `frames_per_call`
    (at 64 frames of the 4096-word vocabulary the optional logits take 1 GB).  to_host=True: uint8 [..., H, W, 3] in pinned host
    memory instead (`egress.frames_to_uint8` per chunk), each chunk downloaded on a side stream behind the next chunk's generation.
    fused=True (with soft=True): the soft image from the soft rows of the fused token step, no [.., V] buffer (`render_slots(fused=True)`);
    sample=True: tokens drawn from softmax(logits / temperature) inside the step.  With either, one `seed` / `sample_seed` (default: fresh
    ones) serves the whole call and each chunk passes its first frame's index, so the chunked video has the bits of one `render` call
    (the noise index frames * tokens * V must stay below 2^32 -- under 1024 frames of 1024 tokens at V 4096 -- and the library refuses more)."""
    from . import egress, steve_render
    lead = tuple(slots.shape[:-2])
    assert slots.dim() in (3, 4), 'slots are [V, T, N, D] or [T, N, D]'
    flat = slots.reshape((-1, ) + tuple(slots.shape[-2:])).float().to(model.device).contiguous()
    key = 'soft' if soft else 'hard'
    F_ = flat.shape[0]
    out, copies, keep = None, None, []
    kw = {}
    if fused or sample:
        kw = dict(fused=fused, sample=sample, temperature=temperature,
                  seed=steve_render._fresh_seed() if seed is None else seed,
                  sample_seed=steve_render._fresh_seed() if sample_seed is None else sample_seed)
    elif seed is not None:
        kw = dict(seed=seed)
    for a, b in render_chunks(F_, frames_per_call):
        if fused or sample:
            kw['first_frame'] = a
        frames = model.render(flat[a:b], soft=soft, **kw)[key]
        if not to_host:
            if out is None:
                out = torch.empty((F_, ) + tuple(frames.shape[1:]), dtype=torch.float32, device=frames.device)
            out[a:b] = frames
            continue
        u8 = egress.frames_to_uint8(frames)
        if out is None:
            out = torch.empty((F_, ) + tuple(u8.shape[1:]), dtype=torch.uint8, pin_memory=True)
            copies = torch.cuda.Stream(device=frames.device)
        ready = torch.cuda.Event()
        ready.record()
        copies.wait_event(ready)
        with torch.cuda.stream(copies):
            out[a:b].copy_(u8, non_blocking=True)
        keep.append(u8)   # alive until its copy has run
    if out is None:
        raise ValueError('slotformer_amd.harness: render_video_slots needs at least one frame')
    if to_host:
        copies.synchronize()
    return out.reshape(lead + tuple(out.shape[1:]))


@torch.no_grad()
def encode_then_rollout(savi, slotformer, img0, vid_len, noise=None):
    """H3 -- test_phyre_planning.py:159-174: SAVi on the first frame(s), zero-pad to `vid_len`,
    SlotFormer forward, all on device.  img0 [B, T0, 3, H, W]."""
    data = {'img': img0.float().to(savi.device)}
    if noise is not None:
        data['noise'] = noise.to(savi.device)
    slot0 = savi(data)['post_slots']
    B, T0, N, C = slot0.shape
    slots = torch.zeros(B, vid_len, N, C, device=slot0.device)
    slots[:, :T0] = slot0
    slotformer.rollout_len = vid_len - slotformer.history_len
    return slotformer({'slots': slots})


_PIPES = {}   # (id(savi), id(rollouter), batch, burn-in, pred_len, options) -> (weakrefs, pipeline): graphs are captured once
# Pipelines kept alive between calls.  Every pipeline owns five or more hardware queues (CU-masked and plain streams), and idle queues
# are not free on this platform: with a second pipeline object alive the same run took 120 instead of 94 ms (profiles/r03_probes.txt
# section 10) -- so by default only the most recently used one is kept; a caller alternating between shapes may raise this.
MAX_PIPELINES = 1


def _pipeline_for(savi, rollouter, batch_size, T, pred_len, pipe_kw):
    import weakref
    from .pipeline import EncodeRolloutPipeline
    for k in [k for k, (ws, wr, _) in _PIPES.items() if ws() is None or wr() is None]:
        _PIPES.pop(k)[2].close()
    key = (id(savi), id(rollouter), batch_size, T, pred_len, tuple(sorted((k, id(v) if isinstance(v, torch.nn.Module) else repr(v)) for k, v in pipe_kw.items())))
    ent = _PIPES.pop(key, None)
    if ent is None:
        while len(_PIPES) >= max(1, MAX_PIPELINES):      # least recently used first (dicts keep insertion order)
            _PIPES.pop(next(iter(_PIPES)))[2].close()
        ent = (weakref.ref(savi), weakref.ref(rollouter), EncodeRolloutPipeline(savi, rollouter, batch_size, T, pred_len, **pipe_kw))
    _PIPES[key] = ent                                      # (re-inserted: most recently used last)
    return ent[2]


def release_pipelines():
    """Close the pipelines extract_and_rollout keeps between calls (graphs, CU-masked streams, workspaces)."""
    for k in list(_PIPES):
        _PIPES.pop(k)[2].close()


@torch.no_grad()
def extract_and_rollout(savi, rollouter, videos, pred_len, batch_size=32, noises=None, pipelined=True, to_host=False, decoder=None,
                        seg_dtype=torch.uint8, encode_group=None, ingest=None, **pipe_kw):
    """Whole hot path over many videos: SAVi slot extraction of the burn-in frames followed by the SlotFormer rollout
    (extract_slots.py:19-38 + rollout_clevrer_slots.py:20-65 / test_phyre_planning.py:159-174 as one on-device call).

    videos [V, T_burn, 3, H, W]: a device tensor, or a HOST tensor -- then the frames stay on the host and are uploaded batch by
    batch by the pipeline's copy stage ahead of the encode, never the whole set at once (pinned input is copied straight from where it
    lies -- the fast path; pageable input passes through a small ring of page-locked staging buffers, one host memcpy per batch).  rollouter: the
    SlotRollouter / SingleStepSlotRollouter container (e.g. `slotformer.rollouter`).  Returns slots [V, T_burn + pred_len,
    N, D] on the device, or in pinned host memory with to_host=True (downloaded behind each rollout; what the reference's
    drivers do before pickling, extract_slots.py:36).  Full batches go through `pipeline.EncodeRolloutPipeline` (kept
    between calls: the rollout graphs are captured once per (models, shape)); a ragged last batch runs serially through the
    same kernels.  `noises` [V, T_burn, N, D] fixes the kernel noise (default: fresh N(0,1) per frame as the reference
    draws it; ignored by models that sample nothing).
    decoder: a module holding the SAVi decoder (the StoSAVi, or the SlotFormer that copied its weights) -- the PREDICTED frames are then
    also decoded behind their rollout (test_vp.py:55-63,145-146: reconstruction + postproc_mask segmentation) and the call returns
    (slots, {'recon': [V, pred_len, 3, R, R] float32, 'seg': [V, pred_len, R, R] seg_dtype}) on the device.  With to_host=True the dict holds
    {'recon_u8': [V, pred_len, R, R, 3] uint8, 'seg': [V, pred_len, R, R] seg_dtype} in pinned host memory instead: the frames as a video writer
    takes them (egress.frames_to_uint8 of the reconstruction), quantised on the device and downloaded behind each decode -- a quarter of the float32
    bytes, and no float32 buffer for the whole set anywhere.
    ingest: an `ingest.FrameIngest` -- `videos` is then the decoder's RAW uint8 clips [V, T_burn, H0, W0, 3] ([V, T_burn, H0, W0] colour indices with
    a palette), on the device or on the host: normalising and resizing (the reference's BaseTransforms) run on the device, batch by batch on the
    pipeline's copy stage, and the uploads carry uint8 at source size.  Anything but uint8 raises ValueError."""
    from . import engine
    dev = next(rollouter.parameters()).device
    if ingest is None:
        videos = videos.float()
    else:
        ingest.output_shape(videos)   # (raises for anything but contiguous uint8 frames: no silent 0..255 floats)
        if videos.dim() != (4 if ingest.palette is not None else 5):
            raise ValueError(f'slotformer_amd: ingest= takes clips [V, T, H0, W0, 3] ([V, T, H0, W0] with a palette), got {tuple(videos.shape)}')
    host_in = not videos.is_cuda
    if host_in:
        videos = videos.contiguous()   # (pageable input is staged batch by batch through the pipeline's ring of page-locked buffers)
    V, T = videos.shape[:2]
    N, D = rollouter.num_slots, rollouter.in_proj.in_features
    # (the decode stage reads the slots from a device-resident `out`: with decoder= and to_host=True they are downloaded at the end)
    out = torch.empty(V, T + pred_len, N, D, pin_memory=True) if to_host and decoder is None else torch.empty(V, T + pred_len, N, D, device=dev)
    # small batches are handed to the pipeline several at a time (pipeline.encode_group_for: the latency-bound slot branch of an encode costs the
    # same for 16 videos as for 32); the kernels are per video, so the slots do not depend on the grouping in the row forms
    # (token-stationary units of >= 96 videos: to ~5e-6)
    from .pipeline import encode_group_for
    # (encode_group: None = that rule; 1 = every batch by itself; the rule depends on V only through 'does the run leave >= 8 pipeline batches')
    if encode_group is None:
        encode_group = encode_group_for(batch_size, V // batch_size) if pipelined and not pipe_kw.get('group') else 1
    batch_size = batch_size * max(1, int(encode_group))
    nfull = V // batch_size
    tail_opts = None
    dec = None
    if decoder is not None:
        R = engine.decoder_plan(decoder).struct.resolution
        if to_host:
            dec = {'recon_u8': torch.empty(V, pred_len, R, R, 3, dtype=torch.uint8, pin_memory=True),
                   'seg': torch.empty(V, pred_len, R, R, dtype=seg_dtype, pin_memory=True)}
        else:
            dec = {'recon': torch.empty(V, pred_len, 3, R, R, device=dev), 'seg': torch.empty(V, pred_len, R, R, device=dev, dtype=seg_dtype)}
        pipe_kw = dict(pipe_kw, decoder=decoder, seg_dtype=seg_dtype)
    if nfull:
        if 'group' not in pipe_kw and pipe_kw.get('partition', 'pair') == 'pair':
            from .pipeline import unit_batches_for
            g = unit_batches_for(rollouter, batch_size, nfull, T)   # long runs of small batches: larger rollout units
            if g:
                pipe_kw = dict(pipe_kw, group=g)
        pipe = _pipeline_for(savi, rollouter, batch_size, T, pred_len, pipe_kw)
        tail_opts = getattr(pipe, 'row_opts', pipe.rollout_opts)   # the ragged tail runs the kernel forms of the full batches (the row-tile ones where those are token-stationary)
        imgs = [videos[j * batch_size:(j + 1) * batch_size] for j in range(nfull)]
        nz = None if noises is None else [noises[j * batch_size:(j + 1) * batch_size].float().to(dev).contiguous() for j in range(nfull)]
        dv = None if dec is None else {k: v[:nfull * batch_size].view(nfull, batch_size, *v.shape[1:]) for k, v in dec.items()}
        pipe.run(imgs, nz, out=out[:nfull * batch_size].view(nfull, batch_size, T + pred_len, N, D), serial=not pipelined or nfull < 2, decoded=dv, ingest=ingest)
    r0 = nfull * batch_size
    if r0 < V:
        nz = None if noises is None else noises[r0:].float().to(dev).contiguous()
        nz = engine.kernel_noise(savi, nz, V - r0, T, dev)   # None for models that sample nothing (kld_method 'none')
        tail_in = videos[r0:].to(dev).contiguous()
        if ingest is not None:
            tail_in = ingest(tail_in)
        post, _, _ = engine.savi_encode(savi, tail_in, noise=nz)
        tail = torch.zeros(V - r0, T + pred_len, N, D, device=dev)
        tail[:, :T] = post
        engine.rollout(rollouter, tail, T, pred_len, opts=tail_opts)
        out[r0:].copy_(tail)
        if dec is not None and not to_host:
            engine.savi_decode(decoder, tail[:, T:].reshape((V - r0) * pred_len, N, D), want=('seg', ), seg_dtype=seg_dtype,
                               out_recon=dec['recon'][r0:].view((V - r0) * pred_len, 3, R, R), out_seg=dec['seg'][r0:].view((V - r0) * pred_len, R, R))
        elif dec is not None:
            from . import egress
            recon = torch.empty(V - r0, pred_len, 3, R, R, device=dev)
            seg = torch.empty(V - r0, pred_len, R, R, device=dev, dtype=seg_dtype)
            engine.savi_decode(decoder, tail[:, T:].reshape((V - r0) * pred_len, N, D), want=('seg', ), seg_dtype=seg_dtype,
                               out_recon=recon.view((V - r0) * pred_len, 3, R, R), out_seg=seg.view((V - r0) * pred_len, R, R))
            dec['recon_u8'][r0:].copy_(egress.frames_to_uint8(recon), non_blocking=True)   # (the same kernel as the pipeline's decode stage)
            dec['seg'][r0:].copy_(seg, non_blocking=True)
    if to_host and dec is not None:
        host = torch.empty(V, T + pred_len, N, D, pin_memory=True)
        host.copy_(out, non_blocking=True)
        out = host
    if to_host:
        torch.cuda.synchronize(dev)
    return out if dec is None else (out, dec)


@torch.no_grad()
def readout_video_slots(readout, slots, batch_size, video_len=75, to_host=True):
    """The contact probability of every video of slots [V, T, N, C] as `rollout_video_slots` returns them (on the device or on the host):
    sigmoid of the `PhysionReadout` logit over the first `video_len` frames, float32 [V] -- in pinned host memory with to_host=True, on the device
    otherwise.  The videos go through in chunks of `batch_size` (the last one may be ragged); a device-resident tensor is read in place through
    its strides, of a host-resident one only a chunk is on the device at a time."""
    if int(batch_size) < 1:
        raise ValueError(f'slotformer_amd.harness: batch_size >= 1, got {batch_size!r}')
    if slots.dim() != 4:
        raise ValueError(f'slotformer_amd.harness: slots are [V, T, N, C], got {tuple(slots.shape)}')
    readout.eval()
    dev = readout.device
    V = slots.shape[0]
    probs = torch.empty(V, dtype=torch.float32, device=dev)
    for a, b in render_chunks(V, int(batch_size)):
        chunk = slots[a:b, :video_len].float().to(dev, non_blocking=True)
        torch.sigmoid(readout({'slots': chunk})['logits'], out=probs[a:b])
    if not to_host:
        return probs
    out = torch.empty(V, dtype=torch.float32, pin_memory=True)
    out.copy_(probs)
    return out


@torch.no_grad()
def phyre_plan(savi, slotformer, readout, frames, statuses=None, batch_size=128, ingest=None, reference_indexing=True, to_host=True):
    """The inference loop of test_phyre_planning.py for V candidate actions: first frame -> SAVi slots -> single-step rollout -> task-success
    classifier -> sigmoid.  frames [V, 1, 3, H, W] (with ingest=, an `ingest.FrameIngest`: the raw uint8 first frames [V, 1, H0, W0, 3], or PHYRE's
    colour indices [V, 1, H0, W0] with a palette), on the device or on the host; statuses [V] (phyre's SimulationStatus, optional): actions with
    INVALID_INPUT (0) are neither encoded nor rolled out and get the confidence -1, as the reference pads them.  Returns conf [V] float32 -- in
    pinned host memory with to_host=True, on the device otherwise.

    The valid actions go through `extract_and_rollout` (`batch_size` actions per encode / rollout batch) with pred_len = max(sel_slots); the
    rolled-out slots stay on the device and go through `readout` (a PHYREReadout) in chunks of `batch_size`, read in place; the head kernel
    writes every confidence straight to its place in conf.

    reference_indexing=True reproduces what test_phyre_planning.py really feeds the classifier: SingleStepSlotFormer.forward classifies
    cat(gt_slots, pred_slots), and in planning gt_slots are the zero frames the first frame was padded with -- so with vid_len = max(sel_slots) + 1
    an index s < vid_len - 1 reads a frame of ZEROS and an index s >= vid_len - 1 reads prediction s - (vid_len - 1); sel_slots [0, 3] reads
    [zeros, the first prediction].  Nothing is concatenated: the kernel takes a frame table with -1 for a zero frame
    (`phyre_planning.frame_table`).  reference_indexing=False indexes [slot0, predictions] instead -- frame 0 is the encoded first frame, frame s
    the prediction s - 1 --, which is what the classifier was trained on (rollout_phyre_slots.py)."""
    from . import phyre_planning as pp
    if int(batch_size) < 1:
        raise ValueError(f'slotformer_amd.harness: batch_size >= 1, got {batch_size!r}')
    if frames.dim() < 2 or frames.shape[1] != 1:
        raise ValueError(f'slotformer_amd.harness: phyre_plan takes the FIRST frame of every action, [V, 1, ...], got {tuple(frames.shape)}')
    readout.eval()
    dev = readout.device
    if dev.type != 'cuda':
        raise RuntimeError('slotformer_amd: phyre_plan runs on a HIP device only; there is no CPU fallback')
    V = frames.shape[0]
    table = pp.frame_table(readout.sel_slots, reference_indexing)
    conf = torch.full((V, ), pp.INVALID_CONF, dtype=torch.float32, device=dev)
    if statuses is None:
        index = torch.arange(V)
    else:
        statuses = torch.as_tensor(statuses).flatten().cpu()
        if statuses.numel() != V:
            raise ValueError(f'slotformer_amd.harness: {V} first frames, {statuses.numel()} statuses')
        index = torch.nonzero(statuses != pp.INVALID_INPUT).flatten()
    if index.numel():
        valid = frames if index.numel() == V else frames[index.to(frames.device)]
        slots = extract_and_rollout(savi, slotformer.rollouter, valid, max(readout.sel_slots), batch_size=int(batch_size), ingest=ingest)
        index = index.to(dev, torch.int32)
        for a, b in render_chunks(index.numel(), int(batch_size)):
            readout.logits_of(slots[a:b], sel=table, scatter_index=index[a:b], scatter_table=conf)
    if not to_host:
        return conf
    out = torch.empty(V, dtype=torch.float32, pin_memory=True)
    out.copy_(conf)
    return out


@torch.no_grad()
def clevrer_answers(model, slots, questions, batch_size=256, to_host=True):
    """The inference loop of test_clevrer_vqa.py without its file I/O: slots [V, T_all, N, C] on the device (the rolled-out CLEVRER slots, read in
    place), questions: the collated arrays -- `cls_q_tokens`, `cls_q_pad_mask` [B1, L], `cls_video_index`, `cls_start` [B1]; `mc_q_tokens`,
    `mc_q_pad_mask` [Bn, L], `mc_flag` [Bn] (the question of every choice, non-decreasing), `mc_video_index`, `mc_start` [B2] (per QUESTION: the
    video of a choice is video_index[mc_flag], an index composition); `frame_offset` and `num_frames` (datasets/clevrer.py: _get_slots reads
    frames start + t * frame_offset; the caller applies the predictive-question shift to the start frames).  A kind may be absent or empty.
    Returns (descriptive answer ids [B1] int32, per-choice booleans [Bn]) -- in pinned host memory with to_host=True, on the device otherwise;
    `clevrer_vqa.result_records` assembles the reference's records from them.  `batch_size` sequences per forward, the last batch ragged."""
    if int(batch_size) < 1:
        raise ValueError(f'slotformer_amd.harness: batch_size >= 1, got {batch_size!r}')
    model.eval()
    dev = model.device
    if dev.type != 'cuda' or not (torch.is_tensor(slots) and slots.is_cuda):
        raise RuntimeError('slotformer_amd: clevrer_answers runs on a HIP device only; there is no CPU fallback')
    tm = model.transformer_model
    offset, frames = int(questions.get('frame_offset', 1)), questions.get('num_frames')

    def on_dev(key, dtype):
        v = questions.get(key)
        return None if v is None else torch.as_tensor(v).to(dev, dtype)

    out = []
    for kind in ('cls', 'mc'):
        tokens, pad = on_dev(f'{kind}_q_tokens', torch.int32), on_dev(f'{kind}_q_pad_mask', torch.uint8)
        n = 0 if tokens is None else tokens.shape[0]
        ans = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            vidx, start = on_dev(f'{kind}_video_index', torch.int64), on_dev(f'{kind}_start', torch.int64)
            if kind == 'mc':
                flag = on_dev('mc_flag', torch.int64)
                vidx, start = vidx[flag], None if start is None else start[flag]
            for a, b in render_chunks(n, int(batch_size)):
                _, got = tm.answer(slots, tokens[a:b], pad[a:b], kind == 'mc', video_index=vidx[a:b], start=None if start is None else start[a:b],
                                   frame_offset=offset, num_frames=frames, want_answers=True)
                ans[a:b] = got
        out.append(ans if kind == 'cls' else ans > 0)
    if not to_host:
        return tuple(out)
    host = tuple(torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in out)
    for h, t in zip(host, out):
        h.copy_(t)
    return host


VP_METRICS = ('mse', 'psnr', 'ssim', 'percept_dist', 'ari', 'fari', 'miou', 'ap', 'ar')   # the arrays test_vp.py saves, plus 'ap'


@torch.no_grad()
def evaluate_video_prediction(model, slots, frames, rollout_len=None, batch_size=8, ingest=None, annotations=None, gt=None, lpips=None,
                              eval_traj=None, max_n_objects=6):
    """The loop of video_prediction/test_vp.py:139-163, 211-219 without its file I/O: per batch of `batch_size` videos (the last one may be ragged)
    the burn-in slots are rolled out, the predicted slots decoded to frames and a uint8 segmentation, the predicted boxes taken from it, and the
    batch scored by `vp_utils.pred_eval_step_device`; the per-step means are accumulated over the batches weighted by the batch size
    (AverageMeter.update(val, B): sum += val * B) in float64 ON THE DEVICE.  No host synchronisation and no download inside the loop; one download
    at the end.

    model: a SlotFormer in eval mode (its rollouter and its StoSAVi decoder).  slots [V, T_total, N, C], the stored slots, on the host or on the
    device: only the first `history_len` frames are read.  frames [V, T_total, 3, R, R] float32 in [-1, 1], or with ingest= (an
    `ingest.FrameIngest`) the raw uint8 clips [V, T_total, H0, W0, 3]; only frames [history_len, history_len + rollout_len) are read.
    rollout_len: default T_total - history_len.  The ground truth of the trajectory scores, over the same T_total frames: annotations= the
    nested list [V][T_total] of per-frame run-length masks of `annotations.pack_frames`, packed once, uploaded ahead of the loop and expanded
    per batch by `annotations.ground_truth` at the resolution of `ingest` (without ingest=: at R x R); or gt= {'mask' [V, T_total, R, R] int64,
    'pres_mask' [V, T_total, M] bool, 'bbox' [V, T_total, M, 4] float32}, ready tensors.  eval_traj: default 'a ground truth was given'; without
    (OBJ3D) the five trajectory scores are zeros, as in the reference.  lpips: a `slotformer_amd.lpips.LPIPS`, or None: 'percept_dist' is then
    0.0, as `pred_eval_step` has it.

    Returns {'mse', 'psnr', 'ssim', 'percept_dist', 'ari', 'fari', 'miou', 'ap', 'ar': np.float64 [rollout_len], 'num_videos': V}.  A step mean
    that is NaN ('ap' / 'ar' of a batch with a frame without boxes) makes that entry NaN for good, as the reference's AverageMeter does.
    RuntimeError when a mask id lay outside [0, 16), as `pred_eval_step` raises -- read from the one download, after the loop."""
    from . import engine
    from . import annotations as ann
    from .video_prediction import vp_utils
    if int(batch_size) < 1:
        raise ValueError(f'slotformer_amd.harness: batch_size >= 1, got {batch_size!r}')
    if annotations is not None and gt is not None:
        raise ValueError('slotformer_amd.harness: annotations= or gt=, not both')
    model.eval()
    dev = model.device
    if dev.type != 'cuda':
        raise RuntimeError('slotformer_amd: evaluate_video_prediction runs on a HIP device only; there is no CPU fallback')
    if slots.dim() != 4:
        raise ValueError(f'slotformer_amd.harness: slots are [V, T_total, N, C], got {tuple(slots.shape)}')
    V, T_total, N, C_ = slots.shape
    hist = model.history_len
    L_ = T_total - hist if rollout_len is None else int(rollout_len)
    if V < 1 or L_ < 1 or hist + L_ > T_total:
        raise ValueError(f'slotformer_amd.harness: {V} videos of {T_total} frames, burn-in {hist}, rollout {L_}')
    if ingest is None:
        if frames.dim() != 5 or tuple(frames.shape[:3]) != (V, T_total, 3):
            raise ValueError(f'slotformer_amd.harness: frames are [{V}, {T_total}, 3, R, R], got {tuple(frames.shape)}')
        from . import ingest as ingest_mod
        mask_ingest = ingest_mod.FrameIngest(tuple(frames.shape[-2:]))   # (only its nearest table is used)
    else:
        shape = ingest.output_shape(frames)   # (raises for anything but contiguous uint8 frames)
        if frames.dim() != (4 if ingest.palette is not None else 5) or tuple(shape[:2]) != (V, T_total):
            raise ValueError(f'slotformer_amd: ingest= takes clips [{V}, {T_total}, H0, W0, 3] ([.., H0, W0] with a palette), got {tuple(frames.shape)}')
        mask_ingest = ingest
    if eval_traj is None:
        eval_traj = annotations is not None or gt is not None
    if eval_traj and annotations is None and gt is None:
        raise ValueError('slotformer_amd.harness: eval_traj needs annotations= or gt=')
    packed = None
    if eval_traj and annotations is not None:
        if len(annotations) != V or any(len(v) != T_total for v in annotations):
            raise ValueError(f'slotformer_amd.harness: annotations are a nested list [{V}][{T_total}] of per-frame object lists')
        packed = ann.pack_frames([list(v[hist:hist + L_]) for v in annotations])   # the frames that are scored, [V][L]
        packed.on(dev)                                                             # uploaded once, ahead of the loop
    elif eval_traj:
        for k, nd in (('mask', 4), ('pres_mask', 3), ('bbox', 4)):
            if k not in gt or gt[k].dim() != nd or tuple(gt[k].shape[:2]) != (V, T_total):
                raise ValueError(f'slotformer_amd.harness: gt= holds mask [V, T_total, R, R], pres_mask [V, T_total, M] and bbox [V, T_total, M, 4]')
    K = len(vp_utils.METRICS)
    acc = torch.zeros((K + 1) * L_ + 2, dtype=torch.float64, device=dev)   # the sums and, behind them, the two flag words: one download
    total = acc[:(K + 1) * L_].view(K + 1, L_)                             # rows of vp_utils.METRICS, then percept_dist
    flags = torch.zeros(2, dtype=torch.int32, device=dev)                  # a mask id outside [0, 16); more non-empty objects than boxes
    for a, b in render_chunks(V, int(batch_size)):
        B = b - a
        clip = torch.empty(B, hist + L_, N, C_, dtype=torch.float32, device=dev)
        clip[:, :hist].copy_(slots[a:b, :hist], non_blocking=True)
        engine.rollout(model.rollouter, clip, hist, L_)
        recon, _, _, seg = engine.savi_decode(model, clip[:, hist:].reshape(B * L_, N, C_), want=('seg', ), seg_dtype=torch.uint8)
        R = recon.shape[-1]
        recon, seg = recon.view(B, L_, 3, R, R), seg.view(B, L_, R, R)
        want = frames[a:b, hist:hist + L_]
        if ingest is None:
            want = want.to(dev, torch.float32, non_blocking=True).contiguous()
        else:
            want = ingest(want.contiguous().to(dev, non_blocking=True))
        if tuple(want.shape) != tuple(recon.shape):
            raise ValueError(f'slotformer_amd.harness: ground-truth frames {tuple(want.shape[-2:])}, decoded frames {R} x {R}')
        kw = {}
        if eval_traj:
            if packed is not None:
                g, over = ann.device_ground_truth(packed.frames(a * L_, b * L_, lead=(B, L_)), mask_ingest, max_n_objects, dev)
                flags[1:] |= over
            else:
                g = {k: gt[k][a:b, hist:hist + L_].to(dev, non_blocking=True) for k in ('mask', 'pres_mask', 'bbox')}
            kw = dict(gt_mask=g['mask'].long(), pred_mask=seg, gt_pres_mask=g['pres_mask'].bool(), gt_bbox=g['bbox'].float(),
                      pred_bbox=vp_utils.masks_to_boxes(seg, model.num_slots))
        out = vp_utils.pred_eval_step_device(want, recon, eval_traj=bool(eval_traj), lpips=lpips, **kw)
        # (the step's result buffers are reused by the next call of this shape: accumulate now)
        total[:K] += torch.stack([out[m] for m in vp_utils.METRICS]) * B
        if lpips is not None:
            total[K] += out['percept_dist'] * B
        flags[:1] |= out['id_out_of_range']
    acc[(K + 1) * L_:] = flags
    host = torch.empty(acc.shape, dtype=torch.float64, pin_memory=True)
    host.copy_(acc, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    if host[-1].item() != 0:
        raise ValueError(f'evaluate_video_prediction: a frame has more than {int(max_n_objects) + 1} non-empty objects (max_n_objects + 1)')
    if host[-2].item() != 0:
        raise RuntimeError('evaluate_video_prediction: a mask id outside [0, 16)')
    avg = host[:(K + 1) * L_].view(K + 1, L_).numpy() / float(V)
    res = {m: avg[i].copy() for i, m in enumerate(vp_utils.METRICS)}
    res['percept_dist'] = avg[K].copy()
    res = {m: res[m] for m in VP_METRICS}
    res['num_videos'] = V
    return res
