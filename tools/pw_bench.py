#!/usr/bin/env python3
"""The tower's 1x1 convolutions on conv_pw.h against the generic kernel (SAYURI_PW=0), in one process.

Synthetic networks written with weights.write_weights: 10 nested-bottleneck blocks at 256 / 128 and at 384 / 192 channels (outer /
inner), and 10 mixer blocks at 256 channels (feed-forward 384).  Per network and point -- default contexts at 1 to 256 boards of
19x19, latency contexts at 1 to 32 boards of 19x19 and one board of 9x9 -- three contexts, interleaved:
  pw0        SAYURI_PW=0: every 1x1 layer on the generic kernel (the code before conv_pw.h)
  pw0_again  the same once more: its ratio to pw0 (`spread`) is what the method cannot tell apart
  pw         the default: conv_pw.h where the engine's speed rule routes it (engine_plan.h, pw_pays)
  pw_all     SAYURI_PW=1: conv_pw.h wherever it applies, the rule not asked -- the rows that show where the rule's boundary belongs
device_ms is the device time per forward, inputs resident (sayuri_hip_time_runs): --warmup forwards, then --rounds rounds of --iters
per context, the MEDIAN of the rounds.  ratio = pw / pw0 and all_ratio = pw_all / pw0; `wins` says whether 1 - ratio exceeds the
spread.  pw_launches / all_launches are sayuri_hip_last_pw_launches of the two arms: 0 where the generic kernel ran.  --pieces a,b
adds an arm per forced SAYURI_PW_PIECES, under SAYURI_PW=1.  Prints ONE JSON object.

    python tools/pw_bench.py > profiles/r12_pw_conv.json
"""
import _ab
from _ab import W

def nested(channels, inner):
    return W.NetSpec(channels, [W.BlockSpec("NestedBottleneckBlock", se=(i % 3 == 2), bottleneck_channels=inner) for i in range(10)], 32, 32)


def mixer(channels, ffn):
    return W.NetSpec(channels, [W.BlockSpec("MixerBlock", se=(i % 3 == 2), ffn_channels=ffn) for i in range(10)], 32, 32)


NETS = {"nested10_256_128": (lambda: nested(256, 128), 41), "nested10_384_192": (lambda: nested(384, 192), 42), "mixer10_256": (lambda: mixer(256, 384), 43)}
POINTS = ([("default", n, 19) for n in (1, 16, 32, 64, 128, 256)] + [("latency", n, 19) for n in (1, 2, 4, 8, 16, 32)] +
          [("latency", 1, 9)])


if __name__ == "__main__":
    _ab.feature_ab("tools/pw_bench.py", NETS, POINTS, "pw", "pieces")
