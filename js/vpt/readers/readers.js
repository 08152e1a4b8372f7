'use strict';
// src/js/readers/{AbstractReader,RAWReader,ZIPReader,BVPReader,ReaderFactory}.js over a loader (js/vpt/loaders).
// Checked against the reference's own readers through tests/golden/readers_r01.json (js/test/test_readers.js).
const { AbstractLoader, BlobLoader } = require('../loaders/loaders.js');

const GL_RED = 6403, GL_R8 = 33321, GL_UNSIGNED_BYTE = 5121;
const GL_RG = 33319, GL_RG8 = 33323;                  // two-channel volumes of BVP manifests
const GL_RGB = 6407, GL_RGB8 = 32849, GL_RGBA = 6408, GL_RGBA8 = 32856;   // byte manifests with more channels (the shaders read .rg)
const GL_FLOAT = 5126, GL_HALF_FLOAT = 5131, GL_R32F = 33326, GL_R16F = 33325;   // float volumes (Volume.js:84-105)
const GL_BYTE = 5120;                                  // signed-normalised volumes (Volume.js:84-105: Int8Array)
const GL_R8_SNORM = 0x8F94, GL_RG8_SNORM = 0x8F95, GL_RGB8_SNORM = 0x8F96, GL_RGBA8_SNORM = 0x8F97;
// packed texel types (Uint16Array / Uint32Array) and the one sized internal format each can be filtered as
const GL_UNSIGNED_SHORT_5_6_5 = 0x8363, GL_RGB565 = 0x8D62, GL_UNSIGNED_SHORT_4_4_4_4 = 0x8033, GL_RGBA4 = 0x8056;
const GL_UNSIGNED_SHORT_5_5_5_1 = 0x8034, GL_RGB5_A1 = 0x8057, GL_UNSIGNED_INT_2_10_10_10_REV = 0x8368, GL_RGB10_A2 = 0x8059;
const GL_UNSIGNED_INT_10F_11F_11F_REV = 0x8C3B, GL_R11F_G11F_B10F = 0x8C3A, GL_UNSIGNED_INT_5_9_9_9_REV = 0x8C3E, GL_RGB9_E5 = 0x8C3D;
// 16-bit normalised volumes (Volume.js:84-105: Uint16Array / Int16Array), filterable through EXT_texture_norm16
const GL_UNSIGNED_SHORT = 5123, GL_SHORT = 5122;
const GL_R16_EXT = 0x822A, GL_RG16_EXT = 0x822C, GL_RGB16_EXT = 0x8054, GL_RGBA16_EXT = 0x805B;
const GL_R16_SNORM_EXT = 0x8F98, GL_RG16_SNORM_EXT = 0x8F99, GL_RGB16_SNORM_EXT = 0x8F9A, GL_RGBA16_SNORM_EXT = 0x8F9B;

class AbstractReader {                                          // AbstractReader.js:1-15
    constructor(loader) { this._loader = loader; }
    async readMetadata() {}
    async readBlock(block) {}
}

// RAWReader.js:3-70; `loader` may also be the bytes themselves (extension: wrapped in a BlobLoader).
// (extension) options `bits` (8 default, 16, 32) and `signed` (16-bit only): the sample type the reference's volume dialog offers and its
// reader drops (VolumeLoadDialog.html:23-34, Application.js:174-179, RAWReader.js:36-38,65-70) — 16: little-endian uint16 (R16_EXT) or,
// signed, int16 (R16_SNORM_EXT), slices of 2 * width * height bytes; 32: little-endian float32 (R32F), 4 * width * height bytes.
class RAWReader extends AbstractReader {

constructor(loader, options) {
    super(loader instanceof AbstractLoader ? loader : new BlobLoader(loader));
    Object.assign(this, { width: 0, height: 0, depth: 0 }, options || {});
    if (this.bits === undefined || this.bits === null) { this.bits = 8; }
    this.signed = !!this.signed;
    if (this.bits !== 8 && this.bits !== 16 && this.bits !== 32) { throw new Error('RAWReader: bits must be 8, 16 or 32, not ' + this.bits); }
    if (this.signed && this.bits !== 16) { throw new Error('RAWReader: signed samples are 16-bit'); }
}

async readMetadata() {                                          // :15-63
    let triple = [GL_RED, GL_R8, GL_UNSIGNED_BYTE];
    if (this.bits === 16) { triple = this.signed ? [GL_RED, GL_R16_SNORM_EXT, GL_SHORT] : [GL_RED, GL_R16_EXT, GL_UNSIGNED_SHORT]; }
    if (this.bits === 32) { triple = [GL_RED, GL_R32F, GL_FLOAT]; }
    const metadata = {
        meta: { version: 1 },
        modalities: [{
            name: 'default',
            dimensions: { width: this.width, height: this.height, depth: this.depth },
            transform: { matrix: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1] },
            format: triple[0], internalFormat: triple[1], type: triple[2],
            placements: [],
        }],
        blocks: [],
    };
    for (let i = 0; i < this.depth; i++) {
        metadata.modalities[0].placements.push({ index: i, position: { x: 0, y: 0, z: i } });
        metadata.blocks.push({ url: 'default', format: 'raw', dimensions: { width: this.width, height: this.height, depth: 1 } });
    }
    return metadata;
}

async readBlock(block) {                                        // :65-70
    const sliceBytes = this.width * this.height * (this.bits >> 3);
    return await this._loader.readData(block * sliceBytes, (block + 1) * sliceBytes);
}

}

// ZIPReader.js:3-100 — stored entries only (the reference returns an entry's bytes as they lie in the archive)
class ZIPReader extends AbstractReader {

constructor(loader) { super(loader); this._eocd = null; this._cd = null; }

async getFiles() {                                              // :13-19
    if (!this._cd) { await this._readCD(); }
    return this._cd.map(entry => entry.name);
}

async readFile(fileName) {                                      // :21-40
    if (!this._cd) { await this._readCD(); }
    const entry = this._cd.find(e => e.name === fileName);
    if (!entry) { throw new Error(`ZIPReader: file ${fileName} not in CD`); }
    const headerEnd = entry.headerOffset + 30;
    const view = new DataView(await this._loader.readData(entry.headerOffset, headerEnd));
    const dataStart = headerEnd + view.getUint16(26, true) + view.getUint16(28, true);
    return await this._loader.readData(dataStart, dataStart + entry.compressedSize);
}

async _readEOCD() {                                             // :42-58
    const MIN_EOCD_SIZE = 22;
    const length = await this._loader.readLength();
    const offset = Math.max(length - MIN_EOCD_SIZE, 0);
    const view = new DataView(await this._loader.readData(offset, offset + Math.min(length, MIN_EOCD_SIZE)));
    this._eocd = { entries: view.getUint16(10, true), size: view.getUint32(12, true), offset: view.getUint32(16, true) };
}

async _readCD() {                                               // :60-93
    if (!this._eocd) { await this._readEOCD(); }
    const data = await this._loader.readData(this._eocd.offset, this._eocd.offset + this._eocd.size);
    const view = new DataView(data), bytes = new Uint8Array(data);
    let offset = 0;
    const entries = [];
    for (let i = 0; i < this._eocd.entries; i++) {
        const nameLength = view.getUint16(offset + 28, true);
        entries.push({
            gpflag: view.getUint16(offset + 8, true),
            method: view.getUint16(offset + 10, true),
            compressedSize: view.getUint32(offset + 20, true),
            uncompressedSize: view.getUint32(offset + 24, true),
            name: Buffer.from(bytes.subarray(offset + 46, offset + 46 + nameLength)).toString('utf8'),
            headerOffset: view.getUint32(offset + 42, true),
        });
        offset += 46 + nameLength + view.getUint16(offset + 30, true) + view.getUint16(offset + 32, true);
    }
    this._cd = entries;
}

}

// BVPReader.js:4-34
class BVPReader extends AbstractReader {

constructor(loader) { super(loader); this._metadata = null; this._zipReader = new ZIPReader(this._loader); }

async readMetadata() {                                          // :13-20
    const data = await this._zipReader.readFile('manifest.json');
    this._metadata = JSON.parse(Buffer.from(data).toString('utf8'));
    return this._metadata;
}

async readBlock(block) {                                        // :22-29
    if (!this._metadata) { await this.readMetadata(); }
    return await this._zipReader.readFile(this._metadata.blocks[block].url);
}

}

function ReaderFactory(which) {                                 // ReaderFactory.js:5-14
    switch (which) {
        case 'bvp': return BVPReader;
        case 'raw': return RAWReader;
        case 'zip': return ZIPReader;
        default: throw new Error('No suitable class');
    }
}

module.exports = { AbstractReader, RAWReader, ZIPReader, BVPReader, ReaderFactory, GL_RED, GL_R8, GL_RG, GL_RG8, GL_UNSIGNED_BYTE,
    GL_RGB, GL_RGB8, GL_RGBA, GL_RGBA8, GL_FLOAT, GL_HALF_FLOAT, GL_R32F, GL_R16F,
    GL_BYTE, GL_R8_SNORM, GL_RG8_SNORM, GL_RGB8_SNORM, GL_RGBA8_SNORM, GL_UNSIGNED_SHORT_5_6_5, GL_RGB565, GL_UNSIGNED_SHORT_4_4_4_4, GL_RGBA4,
    GL_UNSIGNED_SHORT_5_5_5_1, GL_RGB5_A1, GL_UNSIGNED_INT_2_10_10_10_REV, GL_RGB10_A2, GL_UNSIGNED_INT_10F_11F_11F_REV, GL_R11F_G11F_B10F,
    GL_UNSIGNED_INT_5_9_9_9_REV, GL_RGB9_E5, GL_UNSIGNED_SHORT, GL_SHORT, GL_R16_EXT, GL_RG16_EXT, GL_RGB16_EXT, GL_RGBA16_EXT,
    GL_R16_SNORM_EXT, GL_RG16_SNORM_EXT, GL_RGB16_SNORM_EXT, GL_RGBA16_SNORM_EXT };
