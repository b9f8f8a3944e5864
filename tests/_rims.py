"""Sentinel rims round device buffers, shared by the route tests (tests/test_train_routes_gpu.py, test_thin_routes_gpu.py,
test_disc_routes_gpu.py): an output is NaN-filled between GUARD sentinel floats on either side, a workspace 0xff-filled at its stated
size between 256-byte rims of another fill.  An element left unwritten shows as a NaN, a store outside the buffer as a broken rim.
No test in here."""
import torch

DEV = "cuda:0"
NAN = float("nan")
GUARD, SENTINEL = 64, 12345.0          # floats in front of and behind each output (256 bytes: the outputs stay aligned)
BYTE_RIM, BYTE_FILL, BYTE_SENTINEL = 256, 0xFF, 0xA5


def guarded(n):
    """-> (the whole buffer, its NaN-filled middle of n floats)"""
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, device=DEV)
    buf[GUARD:GUARD + n] = NAN
    return buf, buf[GUARD:GUARD + n]


def untouched(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all())


def guarded_bytes(n):
    """-> (the whole byte buffer, its middle of exactly n bytes, every byte 0xff, its first byte at a multiple of 256; the offset of that
    byte): a slab element a kernel should have written and did not is a NaN in the sum"""
    buf = torch.full((BYTE_RIM + n + 2 * BYTE_RIM,), BYTE_SENTINEL, dtype=torch.uint8, device=DEV)
    at = BYTE_RIM + (-(buf.data_ptr() + BYTE_RIM)) % 256
    ws = buf[at:at + n]
    ws.fill_(BYTE_FILL)
    assert ws.data_ptr() % 256 == 0 and ws.numel() == n
    return buf, ws, at


def untouched_bytes(buf, at, n):
    return bool((buf[:at] == BYTE_SENTINEL).all() and (buf[at + n:] == BYTE_SENTINEL).all())
