"""The committed corpus of the differential test (tests/test_graph_gen_cpu.py, tests/test_graph_gen_gpu.py): 48 seeds of tests/graph_gen.py, every
one admitted by graph_gen.admit at its first draw -- a seed that fails admission is simply not listed.  Together they fill the coverage tables
the CPU test prints: the layer table, the planner's decisions and their reasons, the fan-out sweep."""

SEEDS = [1, 38, 43, 61, 62, 87, 100, 129, 167, 168, 173, 194, 196, 230, 236, 240, 250, 253, 257, 267, 272, 293, 317, 321, 326, 329, 338, 346, 348, 354,
         357, 366, 376, 398, 408, 485, 505, 523, 529, 577, 597, 615, 681, 691, 720, 733, 770, 782]

# the graphs that reach a transform-domain conv kernel under the default conv math (a 5-tap 64 -> 64 Conv1D): they run under 'fp32' as well
TRANSFORM = [100, 240, 267, 681, 733]

# what the library cannot run is refused when the layer is built, by name of the constraint -- never in the middle of a step; such a graph is
# not in the corpus.  (what, layer(L), input shape, the message)
REFUSED = [
    ('width-2 Conv2D over a channel pair the strict conv kernels refuse', lambda L: L.Conv2D(3, (3, 5), padding='same'), (8, 2, 3),
     r'Conv2D\(3 filters\) on 3 input channels: the width-2 layer runs as a 6 -> 6 channel Conv1D'),
    ('width-2 Conv2D, one channel to one filter', lambda L: L.Conv2D(1, (5, 5), padding='same'), (8, 2, 1), r'runs as a 2 -> 2 channel Conv1D'),
    ('Conv2D on an image that is not 2 wide', lambda L: L.Conv2D(8, (3, 5), padding='same'), (8, 3, 4), r'width-2 images'),
    ('Conv2DTranspose over a ragged channel pair', lambda L: L.Conv2DTranspose(5, (1, 3)), (4, 4, 6), r'multiples of 4'),
    ('PReLU over a feature count that is no multiple of 4', lambda L: L.PReLU(), (5, 3), r'multiple of 4'),
    ('Conv1D with a stride above 2 on more than 4 channels', lambda L: L.Conv1D(8, 3, strides=3), (16, 8), r'strides 1 and 2'),
]
