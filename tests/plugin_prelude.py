"""What every plugin script (the rows of tests/plugin_scripts.py::CASES) imports in its fresh interpreter: the size scale,
building / loading / registering the shim as three separate steps, and the host <-> HBM round trips over the C Device Data
interface.  Nothing here registers as a side effect and pyarrow.compute is not imported: a script computes the reference's
answers before it registers, and one of them registers before pyarrow.compute exists."""
import ctypes
import os

import pyarrow as pa

EMULATED = os.environ.get("ARROW_AMD_PLUGIN_EMULATED") == "1"      # CPU tier: the shim on the emulated kernels (tests/emu)


def SC(x):
    """A row count of the GPU tier, shrunk by ARROW_AMD_TEST_SCALE for the emulated run."""
    return max(64, int(x * float(os.environ.get("ARROW_AMD_TEST_SCALE", "1"))))


def build():
    """Build the shim (on the emulated kernels in the CPU tier) and return its path."""
    if EMULATED:
        from tests.emu.build_plugin_emu import build_plugin
    else:
        from arrow_amd.plugin_build import build_plugin
    return build_plugin()


def load(path=None):
    """dlopen the shim and type its error / counter readers.  Does not register."""
    lib = ctypes.CDLL(path or build())
    lib.arrow_amd_plugin_last_error.restype = ctypes.c_char_p
    lib.arrow_amd_plugin_calls.restype = ctypes.c_int64
    lib.arrow_amd_plugin_calls.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.arrow_amd_plugin_gpu_calls.restype = ctypes.c_int64
    lib.arrow_amd_plugin_stock_calls.restype = ctypes.c_int64
    return lib


def register(lib):
    assert lib.arrow_amd_register() == 0, lib.arrow_amd_plugin_last_error()


def to_device(lib, arr):
    c_arr, c_schema, c_dev = (ctypes.create_string_buffer(m) for m in (80, 72, 128))
    arr._export_to_c(ctypes.addressof(c_arr), ctypes.addressof(c_schema))
    assert lib.arrow_amd_copy_to_device(c_arr, c_schema, c_dev) == 0, lib.arrow_amd_plugin_last_error()
    return pa.Array._import_from_c_device(ctypes.addressof(c_dev), arr.type)


def to_host(lib, darr):
    """The host copy, imported under the schema the plugin exports (not the caller's type)."""
    c_dev, c_schema, c_arr, c_schema2 = (ctypes.create_string_buffer(m) for m in (128, 72, 80, 72))
    darr._export_to_c_device(ctypes.addressof(c_dev), ctypes.addressof(c_schema))
    assert lib.arrow_amd_copy_to_host(c_dev, c_schema, c_arr, c_schema2) == 0, lib.arrow_amd_plugin_last_error()
    return pa.Array._import_from_c(ctypes.addressof(c_arr), ctypes.addressof(c_schema2))


def device_table(lib, table, batches=3):
    """`table` with every column in HBM, as `batches` record batches."""
    return pa.Table.from_batches([pa.RecordBatch.from_arrays([to_device(lib, c) for c in b.columns], names=b.schema.names)
                                  for b in table.to_batches(max_chunksize=-(-len(table) // batches))])


def calls(lib, name, gpu):
    """How often the shim's kernel of `name` ran on the device (gpu=1) or handed over to the reference's (gpu=0)."""
    return lib.arrow_amd_plugin_calls(name.encode(), gpu)


def single_threaded_when_emulated():
    """The SIMT emulator runs one kernel at a time (one fiber scheduler): one Acero thread.  Thread-local states and Merge
    still happen under use_threads=True, their consumes just never overlap."""
    if EMULATED:
        pa.set_cpu_count(1)
        pa.set_io_thread_count(1)
