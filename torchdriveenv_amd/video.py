"""render_mode="video" of the reference-shaped surface (WaypointSuiteEnv): the frames BirdviewRecordingWrapper(res=video_res,
fov=video_fov, to_cpu=True) records (ref gym_env.py:295-297) and the file GymEnv.close() writes from them through helpers.save_video
(gym_env.py:172-176).  The frames come from ops.render_scene (tde_render_scene); this module holds the list and the writer."""
import os
import warnings

import numpy as np
import torch


def save_video(frames, filename, fps=10):
    """frames: uint8 [1, 3, H, W] tensors -> `filename`, with the conventions of the reference's save_video (helpers.py:7-27): RGB ->
    BGR, HWC, fourcc mp4v, 10 fps, cv2.VideoWriter.  Without cv2 but with PIL an animated GIF is written beside it (same stem, .gif)
    with a warning; with neither, ImportError.  Returns the path written."""
    try:
        import cv2
    except ImportError:
        cv2 = None
    imgs = [np.ascontiguousarray(torch.as_tensor(f)[0].cpu().numpy().astype(np.uint8).transpose(1, 2, 0)) for f in frames]
    if cv2 is not None:
        h, w = imgs[0].shape[:2]
        out = cv2.VideoWriter(filename=filename, fourcc=cv2.VideoWriter_fourcc(*"mp4v"), fps=fps, frameSize=(w, h))
        for im in imgs:
            out.write(np.ascontiguousarray(im[:, :, ::-1]))          # RGB -> BGR (cv2.cvtColor(.., COLOR_RGB2BGR))
        out.release()
        return filename
    try:
        from PIL import Image
    except ImportError:
        raise ImportError(f"writing {filename} needs cv2 (opencv-python), as the reference's save_video does; PIL is not available "
                          "either.  The frames are kept: get_birdviews()") from None
    gif = os.path.splitext(filename)[0] + ".gif"
    warnings.warn(f"cv2 is not available: writing an animated GIF, {gif}, instead of {filename}")
    pics = [Image.fromarray(im) for im in imgs]
    pics[0].save(gif, save_all=True, append_images=pics[1:], duration=int(round(1000 / fps)), loop=0)
    return gif


class VideoRecorder:
    """The frame list of BirdviewRecordingWrapper and GymEnv.close()'s use of it.  The reference rebuilds its simulator - and so
    the wrapper and its list - on every reset: `start()` begins a new list.  A VecEnv that auto-resets an env on its last step
    therefore leaves a one-frame list behind, and close() writes nothing (gym_env.py:175 writes only more than one frame): kept
    as the reference does it."""

    def __init__(self, filename, fps=10):
        self.filename = filename
        self.fps = fps
        self.frames = []

    def start(self):
        self.frames = []

    def append(self, frame):
        self.frames.append(frame)

    def close(self):
        """writes the file when there is more than one frame; returns its path, or None"""
        if len(self.frames) > 1:
            return save_video(self.frames, self.filename, self.fps)
        return None
