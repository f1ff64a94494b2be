"""Restatements of LogMelSpec(sr, n_mels) for any shape (tal/asr/models.py:22-53: n_fft = win = int(0.025 sr),
hop = int(0.01 sr)): the fp32 torch.stft form the reference computes, and a float64 numpy twin (explicit reflect pad + rfft).
Both take the window and the filterbank as given, so checkpoint buffers of any values can be checked."""
import numpy as np
import torch

from oracle import tal_oracle as O


def shape_for(sr):
    """-> (n_fft, hop) of LogMelSpec(sr)."""
    return int(25 / 1000 * sr), int(10 / 1000 * sr)


def buffers(sr, n_mels):
    """-> (window [n_fft], fb [n_fft//2 + 1, n_mels]) as torchaudio builds them (float32)."""
    n_fft, _ = shape_for(sr)
    return O.hann_window(n_fft), O.mel_filterbank(n_fft // 2 + 1, n_mels, sr)


def mel_power_f32(audio, window, fb, hop):
    """torchaudio 0.4.0 MelSpectrogram.forward for any shape: fp32 torch.stft -> power -> fb: [B, L] -> [B, T, n_mels]."""
    a = torch.as_tensor(np.asarray(audio, dtype=np.float32)) if not torch.is_tensor(audio) else audio.float()
    window = torch.as_tensor(window, dtype=torch.float32)
    n_fft = window.shape[0]
    spec = torch.stft(a, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    p = spec.real * spec.real + spec.imag * spec.imag                 # [B, n_fft//2 + 1, T]
    return torch.matmul(p.transpose(1, 2), torch.as_tensor(fb, dtype=torch.float32))


def logmel_f32(audio, window, fb, hop, eps=1e-6, subtract_mean=True):
    """mel_power_f32 -> log(. + eps), minus ONE global mean: [B, L] -> [B, T, n_mels] (torch float32)."""
    mel = torch.log(mel_power_f32(audio, window, fb, hop) + eps)
    if subtract_mean:
        mel = mel - mel.mean()
    return mel


def logmel_f64_frames(audio_1d, window, fb, hop, f0, f1, eps=1e-6):
    """Frames [f0, f1) of log(mel + eps) (NO mean subtraction) of ONE clip in float64 -> [f1 - f0, n_mels]."""
    a = np.asarray(audio_1d, dtype=np.float64)
    win = np.asarray(window, dtype=np.float64)
    n_fft = win.shape[0]
    L = a.shape[0]
    pad = n_fft // 2
    idx = np.arange(f0 * hop - pad, (f1 - 1) * hop + n_fft - pad)
    idx = np.where(idx < 0, -idx, idx)                          # reflect (no edge repeat)
    idx = np.where(idx >= L, 2 * (L - 1) - idx, idx)
    seg = a[idx]
    fi = np.arange(f1 - f0)[:, None] * hop + np.arange(n_fft)[None, :]
    spec = np.fft.rfft(seg[fi] * win, axis=-1)
    power = spec.real ** 2 + spec.imag ** 2
    return np.log(power @ np.asarray(fb, dtype=np.float64) + eps)


def logmel_f64(audio, window, fb, hop, eps=1e-6, subtract_mean=True):
    """Float64 twin of logmel_f32: [B, L] -> [B, T, n_mels] float64."""
    a = np.asarray(audio, dtype=np.float64)
    n_fft = np.asarray(window).shape[0]
    T = 1 + (a.shape[1] + 2 * (n_fft // 2) - n_fft) // hop        # torch.stft's count (center=True)
    mel = np.stack([logmel_f64_frames(row, window, fb, hop, 0, T, eps) for row in a])
    if subtract_mean:
        mel = mel - mel.mean()
    return mel


def hann_f64(n_fft):
    """The periodic Hann window evaluated in float64 (the oracle's float64 restatement uses it)."""
    k = np.arange(n_fft, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * k / n_fft)
