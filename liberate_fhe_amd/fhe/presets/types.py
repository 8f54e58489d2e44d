"""Origin tags carried by every data_struct (reference: src/liberate/fhe/presets/types.py:1-11)."""

origins = dict(
    sk="secret key",
    pk="public key",
    ksk="key switch key",
    rotk="rotation key:",
    galk="galois key",
    conjk="conjugation key",
    ct="cipher text",
    ctt="cipher text triplet",
    diag="plain diagonals:",   # ckks_engine.encode_diagonals: followed by the steps, as a rotation key's tag by its step
    diag_bsgs="plain diagonals bsgs:",   # encode_diagonals(bsgs=n1): followed by "n1;steps", the pack in (giant, baby) order
    pt_mult="plain mult",      # ckks_engine.encode_plain(op="mult"): the plaintext mc_mult builds (NTT domain, Montgomery form)
    pt_mult_planes="plain mult planes",   # compact_plain(pt_mult): fp64-class rows as 6-byte planes of the plain word, one flat tensor per device
    pt_add="plain add",        # encode_plain(op="add"): the plaintext mc_add builds (coefficient domain, Montgomery form)
)
