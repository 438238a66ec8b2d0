"""On-disk slot formats the reference's offline pipeline exchanges (row N3 of SURVEY.md 8f).

* CLEVRER / OBJ3D / Physion: one pickle per dataset, ``{split: {video_basename: float32 [T,N,C]}}``
  (extract_slots.py:57-76, written with nerv ``dump_obj`` = pickle for ``.pkl``); read back by key
  ``os.path.basename(video_path)`` (datasets/clevrer.py:323-335).
* PHYRE: one ``{data_idx:06d}.npy`` per sample holding ``slots[:vid_len]`` (extract_phyre_slots.py:69-76);
  extraction is restartable -- files already present are skipped, the newest one is redone in case it
  was truncated (extract_phyre_slots.py:45-53).
* Physion dVAE tokens: one int16 ``[T, h*w]`` ``.npy`` per video beside the videos (tokenize_images.py:55-66), read back as strided int32 clips
  (datasets/physion.py:81-93); files already present are skipped.
"""
import os
import pickle

import numpy as np


def slots_to_dict(files, slots):
    """files: list of video paths; slots: array-like [V,T,N,C] -> {basename: float32 [T,N,C]}."""
    assert len(files) == len(slots)
    return {os.path.basename(f): np.asarray(s, dtype=np.float32) for f, s in zip(files, slots)}


def dump_slots(path, **splits):
    """dump_slots('slots.pkl', train={...}, val={...}[, test={...}]) -- the reference's pickle layout."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'wb') as f:
        pickle.dump({k: v for k, v in splits.items()}, f)


def link_slots(save_path, weight_path, subset=None):
    """The soft link the reference leaves next to the weights a slot file was extracted with (extract_slots.py:86-93): `<weight dir>/slots.pkl`,
    or `<weight dir>/<subset>_slots.pkl` for the Physion subsets -- where the video-prediction configs look for the slots.  An existing link is
    replaced (the reference's `ln -s` fails silently there); returns the link's path."""
    name = 'slots.pkl' if subset is None else f'{subset}_slots.pkl'
    ln_path = os.path.join(os.path.dirname(os.path.abspath(weight_path)), name)
    if os.path.islink(ln_path):
        os.unlink(ln_path)
    os.symlink(os.path.abspath(save_path), ln_path)
    return ln_path


def load_slots(path):
    with open(path, 'rb') as f:
        return pickle.load(f)


def stack_slot_table(video_slots, names=None):
    """A slot dictionary {name: [T,N,C]} (one split of the pickle above) -> (float32 array [V,T,N,C], names): the table
    `video_prediction.fit` keeps on the device, video v being names[v].  names: the order wanted (default: sorted keys).  Every video must have
    the same shape -- CLEVRER's and OBJ3D's do; pad or bucket Physion's ragged videos first and hand their lengths to `fit` as `clip_len`."""
    names = sorted(video_slots) if names is None else [os.path.basename(n) for n in names]
    if not names:
        raise ValueError('no videos to stack')
    shape = np.shape(video_slots[names[0]])
    if len(shape) != 3:
        raise ValueError(f'the slots of a video are [T, N, C], got {shape}')
    table = np.empty((len(names), ) + tuple(shape), dtype=np.float32)
    for v, n in enumerate(names):
        s = np.asarray(video_slots[n], dtype=np.float32)
        if s.shape != tuple(shape):
            raise ValueError(f'{n}: slots {s.shape}, the table holds {tuple(shape)}')
        table[v] = s
    return table, names


def read_clip(video_slots, video_path, start_idx, n_sample_frames, frame_offset):
    """datasets/clevrer.py:323-335: strided clip [n_sample_frames,N,C] of one video's slots."""
    try:
        slots = video_slots[os.path.basename(video_path)]
    except KeyError:
        raise ValueError(f'no slots for {video_path}')
    return np.stack([slots[start_idx + n * frame_offset] for n in range(n_sample_frames)], 0).astype(np.float32)


def token_path(video_path, dvae_name):
    """Where the dVAE tokens of a Physion video live (tokenize_images.py:57-63, datasets/physion.py:81-85): the video's path with
    `TrainMP4s/` -> `TrainNpys-<dvae_name>/`, `TestMP4s/` -> `TestNpys-<dvae_name>/` and `.mp4` -> `.npy`.  The dataset names a video by its
    frame folder (no extension): `.npy` is then appended, which gives the same file."""
    p = video_path.replace('TrainMP4s/', f'TrainNpys-{dvae_name}/').replace('TestMP4s/', f'TestNpys-{dvae_name}/')
    return p.replace('.mp4', '.npy') if '.mp4' in p else p + '.npy'


def save_video_tokens(files, tokens, dvae_name, overwrite=False):
    """One `[T, h*w]` int16 file per video (tokenize_images.py:55-66) at `token_path(file, dvae_name)`; tokens: array-like [N, T, h*w] (what
    `harness.extract_video_tokens` returns).  A file that already exists is left alone unless `overwrite`, so an interrupted run resumes
    where it stopped; each file is written under a temporary name and renamed, so a crash never leaves a truncated one behind.  Returns the
    paths it wrote."""
    assert len(files) == len(tokens)
    written = []
    for f, t in zip(files, tokens):
        path = token_path(f, dvae_name)
        if os.path.exists(path) and not overwrite:
            continue
        t = np.asarray(t)
        if t.ndim != 2:
            raise ValueError(f'tokens of a video are [T, h*w], got {t.shape}')
        if t.dtype != np.int16 and (t.min() < 0 or t.max() > 32767):
            raise ValueError('token ids do not fit the int16 of the token files')
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = path + '.tmp.npy'
        np.save(tmp, t.astype(np.int16))
        os.replace(tmp, path)
        written.append(path)
    return written


def read_token_clip(path, start_idx, n_sample_frames, frame_offset):
    """datasets/physion.py:81-93: the strided clip [n_sample_frames, h*w] int32 of one video's token file, or None when the file is missing
    (the dataset then leaves `token_id` out and the model tokenises the frames itself)."""
    if not os.path.exists(path):
        return None
    tokens = np.load(path)   # [T, h*w]
    return np.stack([tokens[start_idx + n * frame_offset] for n in range(n_sample_frames)], 0).astype(np.int32)


def phyre_path(save_root, data_idx):
    return os.path.join(save_root, f'{int(data_idx):06d}.npy')


def save_phyre_slots(save_root, data_idx, slots, vid_len):
    """One file per sample, truncated to the real video length (extract_phyre_slots.py:69-76)."""
    os.makedirs(save_root, exist_ok=True)
    np.save(phyre_path(save_root, data_idx), np.asarray(slots, dtype=np.float32)[:int(vid_len)])


def phyre_resume_index(save_root, start, end):
    """First index in [start, end) that still has to be processed (extract_phyre_slots.py:45-53): scan forward, stop at
    the FIRST missing file and redo the one before it (it may have been truncated by the crash).  Files beyond a gap
    are not trusted -- every index from the returned one on is (re)written."""
    idx = start
    while idx < end and os.path.exists(phyre_path(save_root, idx)):
        idx += 1
    return max(idx - 1, start)
